// TEST INFRASTRUCTURE ONLY -- the members of the reference's KeyFrame (include/KeyFrame.h) that include/orbfe/Covisibility.h
// touches, with the behaviour of AddConnection / UpdateBestCovisibles / AddChild (src/KeyFrame.cc:134-170, :404-409) written
// again so that tests/cpp/covisibility_test.cpp can build a small map.  The covisibility members are PROTECTED, as in the
// reference, and opened to the facade by the one friend line an integrator adds to the real header.
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "MapPoint.h"
namespace orbfe { struct CovisibilityAccess; }
namespace ORB_SLAM2 {
class KeyFrame {
 public:
  long unsigned int mnId = 0;
  std::vector<MapPoint*> GetMapPointMatches() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mvpMapPoints; }
  bool isBad() { return mbBad; }
  void AddConnection(KeyFrame* pKF, const int& weight) {
    if (mbBad || pKF->isBad()) return;
    {
      std::unique_lock<std::mutex> lock(mMutexConnections);
      std::map<KeyFrame*, int>::iterator it = mConnectedKeyFrameWeights.find(pKF);
      if (it != mConnectedKeyFrameWeights.end() && it->second == weight) return;
      mConnectedKeyFrameWeights[pKF] = weight;
    }
    UpdateBestCovisibles();
  }
  void UpdateBestCovisibles() {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    std::vector<std::pair<int, KeyFrame*> > vPairs;
    for (std::map<KeyFrame*, int>::iterator it = mConnectedKeyFrameWeights.begin(); it != mConnectedKeyFrameWeights.end(); ++it)
      vPairs.push_back(std::make_pair(it->second, it->first));
    std::sort(vPairs.begin(), vPairs.end());
    mvpOrderedConnectedKeyFrames.clear();
    mvOrderedWeights.clear();
    for (size_t i = vPairs.size(); i-- > 0;) {
      mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second);
      mvOrderedWeights.push_back(vPairs[i].first);
    }
  }
  void AddChild(KeyFrame* pKF) {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if (!mbBad && !pKF->isBad()) mspChildrens.insert(pKF);
  }
  // test side: build the object, read the protected members back
  void testSetMapPoints(const std::vector<MapPoint*>& v) { mvpMapPoints = v; }
  void testSetBad(bool b) { mbBad = b; }
  const std::map<KeyFrame*, int>& testWeights() const { return mConnectedKeyFrameWeights; }
  const std::vector<KeyFrame*>& testOrdered() const { return mvpOrderedConnectedKeyFrames; }
  const std::vector<int>& testOrderedWeights() const { return mvOrderedWeights; }
  KeyFrame* testParent() const { return mpParent; }
  bool testFirstConnection() const { return mbFirstConnection; }
  const std::set<KeyFrame*>& testChildren() const { return mspChildrens; }

 protected:
  friend struct orbfe::CovisibilityAccess;
  friend struct CovisibilityRestated;          // tests/cpp/covisibility_test.cpp: the whole reference function, written again
  std::vector<MapPoint*> mvpMapPoints;
  std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  std::vector<int> mvOrderedWeights;
  bool mbFirstConnection = true;
  KeyFrame* mpParent = nullptr;
  std::set<KeyFrame*> mspChildrens;
  bool mbBad = false;
  std::mutex mMutexConnections;
  std::mutex mMutexFeatures;
};
}  // namespace ORB_SLAM2
