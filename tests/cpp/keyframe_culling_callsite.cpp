// The call site INTEGRATION.md gives for LocalMapping::KeyFrameCulling, type-checked against the stubs (-fsyntax-only).
#include <vector>

#include "KeyFrame.h"
#include "orbfe/KeyFrameCulling.h"

using namespace std;
namespace ORB_SLAM2 {
struct LocalMapping {
  orbfe_matcher* matcher;
  KeyFrame* mpCurrentKeyFrame;
  vector<KeyFrame*> covisibles;
  vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return covisibles; }
  void KeyFrameCulling();
};
void LocalMapping::KeyFrameCulling() {
  vector<KeyFrame*> vpLocalKeyFrames = GetVectorCovisibleKeyFrames();
  orbfe::KeyFrameCulling(matcher, vpLocalKeyFrames);
}
}  // namespace ORB_SLAM2
