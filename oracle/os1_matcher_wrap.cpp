/* os1_matcher_wrap.cpp -- flat C interface of oracle/_ref/libos1_matcher.so: the reference's OWN src/ORBmatcher.cc, compiled
 * unmodified and where it lies (oracle/Makefile) against the stand-in headers of oracle/os1_decl/, one entry per member.  The
 * arguments are those of the oracle's restatements of the same members (oracle/orb_oracle_pose.h and the array forms of
 * oracle/orb_oracle.cpp), so one scene feeds both sides, and every entry returns all a caller of the member can observe.
 * MapPoints are rows of a table, named by their index (-1 = NULL).  TEST INFRASTRUCTURE ONLY. */
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>

#include "ORBmatcher.h"   // the reference's own header, copied beside the three stand-ins at build time (oracle/_ref/os1_inc/)
#include "orb_oracle_pose.h"

using namespace ORB_SLAM2;

namespace {
static_assert(sizeof(cv::KeyPoint) == sizeof(OrcKp), "cv::KeyPoint has the layout of OrcKp");

struct Open : ORBmatcher {   // the two protected helpers
  Open() : ORBmatcher(0.6f, true) {}
  using ORBmatcher::ComputeThreeMaxima;
  using ORBmatcher::RadiusByViewingCos;
};

std::vector<cv::KeyPoint> keys(const OrcKp* k, int n) {
  std::vector<cv::KeyPoint> v(n);
  if (n) std::memcpy(v.data(), k, (size_t)n * sizeof(OrcKp));
  return v;
}
cv::Mat descRows(const uint8_t* d, int n) { return cv::Mat(n, 32, CV_8U, d); }
cv::Mat identity4() {
  cv::Mat T(4, 4, CV_32F);
  for (int i = 0; i < 4; i++) T.at<float>(i, i) = 1.f;
  return T;
}

template <class V> void fillView(V& f, const OrcView* v) {
  f.N = v->n;
  f.mvKeysUn = keys(v->kpsUn, v->n);
  f.mvKeys = f.mvKeysUn;
  f.mDescriptors = descRows(v->desc, v->n);
  f.mvpMapPoints.assign(v->n, static_cast<MapPoint*>(NULL));
  f.mnMinX = v->bounds[0]; f.mnMaxX = v->bounds[1]; f.mnMinY = v->bounds[2]; f.mnMaxY = v->bounds[3];
  f.fx = v->fx; f.fy = v->fy; f.cx = v->cx; f.cy = v->cy;
  f.mvScaleFactors.assign(v->scaleFactors, v->scaleFactors + v->nlevels);
  if (v->invLevelSigma2) f.mvInvLevelSigma2.assign(v->invLevelSigma2, v->invLevelSigma2 + v->nlevels);
  f.mfLogScaleFactor = v->logScaleFactor;
  f.AssignFeaturesToGrid();
}

struct Table {   // OrcPoints as MapPoint objects, written back on destruction
  OrcPoints* P;
  std::vector<MapPoint> mp;
  Table(OrcPoints* P_, KeyFrame* obsKF) : P(P_), mp(P_->M) {
    for (int i = 0; i < P->M; i++) {
      MapPoint& m = mp[i];
      m.id = i;
      m.mWorldPos = cv::Mat(3, 1, CV_32F, P->pos + 3 * i);
      if (P->normal) m.mNormalVector = cv::Mat(3, 1, CV_32F, P->normal + 3 * i);
      m.mDescriptor = cv::Mat(1, 32, CV_8U, P->desc + 32 * (size_t)i);
      m.mfMinDistance = P->mfMinDistance[i];
      m.mfMaxDistance = P->mfMaxDistance[i];
      m.mbBad = P->bad[i] != 0;
      m.nObs = P->nObs[i];
      m.idxInKF = P->idxInKF[i];
      m.obsKF = obsKF;
    }
  }
  ~Table() {
    for (int i = 0; i < P->M; i++) {
      P->bad[i] = mp[i].mbBad ? 1 : 0;
      P->nObs[i] = mp[i].nObs;
      P->idxInKF[i] = mp[i].idxInKF;
    }
  }
  MapPoint* at(int id) { return id < 0 ? static_cast<MapPoint*>(NULL) : &mp[id]; }
  std::vector<MapPoint*> list(const int32_t* ids, int n) {
    std::vector<MapPoint*> v(n);
    for (int i = 0; i < n; i++) v[i] = at(ids[i]);
    return v;
  }
};
void ids(const std::vector<MapPoint*>& v, int32_t* out) {
  for (size_t i = 0; i < v.size(); i++) out[i] = v[i] ? v[i]->id : -1;
}

DBoW2::FeatureVector featVec(const uint32_t* nodes, const uint32_t* off, const uint32_t* feat, int nfv) {
  DBoW2::FeatureVector fv;
  for (int a = 0; a < nfv; a++)
    for (uint32_t j = off[a]; j < off[a + 1]; j++) fv.addFeature(nodes[a], feat[j]);
  return fv;
}
}  // namespace

extern "C" {

int os1_matcher_is_reference_build() { return 1; }   // (tools/gen_os1_matcher_golden.py asks before it writes)
void os1_matcher_constants(int out[3]) { out[0] = ORBmatcher::TH_HIGH; out[1] = ORBmatcher::TH_LOW; out[2] = ORBmatcher::HISTO_LENGTH; }

int os1_descriptor_distance(const uint8_t* a, const uint8_t* b) {
  return ORBmatcher::DescriptorDistance(cv::Mat(1, 32, CV_8U, a), cv::Mat(1, 32, CV_8U, b));
}
// DescriptorDistance(D.row(ia), D.row(ib)) on the views of one n x 32 matrix, as every search calls it
int os1_descriptor_distance_rows(const uint8_t* rows, int n, int ia, int ib) {
  const cv::Mat D = descRows(rows, n);
  return ORBmatcher::DescriptorDistance(D.row(ia), D.row(ib));
}
float os1_radius_by_viewing_cos(float viewCos) { return Open().RadiusByViewingCos(viewCos); }
// histo[i] has counts[i] entries; ind (in/out) = ind1, ind2, ind3
void os1_compute_three_maxima(const int* counts, int L, int ind[3]) {
  std::vector<std::vector<int> > h(L);
  for (int i = 0; i < L; i++) h[i].assign(counts[i], 0);
  Open().ComputeThreeMaxima(h.data(), L, ind[0], ind[1], ind[2]);
}

// SearchByProjection(Frame&, const vector<MapPoint*>&, th); arguments of orc_search_by_projection
int os1_search_by_projection(const OrcKp* kpsUn, const uint8_t* desc, int n, const float bounds[4], const float* mvScaleFactors,
                             const uint8_t* kp_occupied, const float* mp_proj_xy, const int* mp_level, const float* mp_viewcos,
                             const uint8_t* mp_flags, const uint8_t* mp_desc, int n_mp, float th, float mfNNratio, int* kp_assigned) {
  int nlev = 1;
  for (int i = 0; i < n_mp; i++) nlev = std::max(nlev, mp_level[i] + 1);
  OrcView v;
  std::memset(&v, 0, sizeof v);
  v.kpsUn = kpsUn; v.desc = desc; v.n = n; v.scaleFactors = mvScaleFactors; v.nlevels = nlev;
  std::memcpy(v.bounds, bounds, sizeof v.bounds);
  Frame F;
  fillView(F, &v);
  MapPoint holder;   // what an occupied keypoint holds: a MapPoint with an observation
  holder.nObs = 1;
  for (int i = 0; i < n; i++)
    if (kp_occupied[i]) F.mvpMapPoints[i] = &holder;
  std::vector<MapPoint> mp(n_mp);
  std::vector<MapPoint*> vp(n_mp);
  for (int i = 0; i < n_mp; i++) {
    MapPoint& m = mp[i];
    m.id = i;
    m.mbTrackInView = mp_flags[i] & 1;
    m.mbBad = (mp_flags[i] & 2) != 0;
    m.plCandidato = (mp_flags[i] & 4) != 0;
    m.nObs = (mp_flags[i] & 8) ? 1 : 0;
    m.mTrackProjX = mp_proj_xy[2 * i]; m.mTrackProjY = mp_proj_xy[2 * i + 1];
    m.mnTrackScaleLevel = mp_level[i];
    m.mTrackViewCos = mp_viewcos[i];
    m.mDescriptor = cv::Mat(1, 32, CV_8U, mp_desc + 32 * (size_t)i);
    vp[i] = &m;
  }
  ORBmatcher matcher(mfNNratio, true);
  const int r = matcher.SearchByProjection(F, vp, th);
  ids(F.mvpMapPoints, kp_assigned);
  return r;
}

// SearchForInitialization; arguments of orc_search_for_initialization (prev_xy = vbPrevMatched, in/out)
int os1_search_for_initialization(const OrcKp* kps1, const uint8_t* desc1, int n1, const OrcKp* kps2, const uint8_t* desc2, int n2,
                                  const float bounds[4], float* prev_xy, int* vnMatches12, int windowSize, float mfNNratio,
                                  int mbCheckOrientation) {
  Frame F1, F2;
  F1.N = n1; F1.mvKeysUn = keys(kps1, n1); F1.mvKeys = F1.mvKeysUn; F1.mDescriptors = descRows(desc1, n1);
  F2.N = n2; F2.mvKeysUn = keys(kps2, n2); F2.mvKeys = F2.mvKeysUn; F2.mDescriptors = descRows(desc2, n2);
  F2.mnMinX = bounds[0]; F2.mnMaxX = bounds[1]; F2.mnMinY = bounds[2]; F2.mnMaxY = bounds[3];
  F2.AssignFeaturesToGrid();
  std::vector<cv::Point2f> prev(n1);
  for (int i = 0; i < n1; i++) prev[i] = cv::Point2f(prev_xy[2 * i], prev_xy[2 * i + 1]);
  std::vector<int> m12;
  ORBmatcher matcher(mfNNratio, mbCheckOrientation != 0);
  const int r = matcher.SearchForInitialization(F1, F2, prev, m12, windowSize);
  for (int i = 0; i < n1; i++) { vnMatches12[i] = m12[i]; prev_xy[2 * i] = prev[i].x; prev_xy[2 * i + 1] = prev[i].y; }
  return r;
}

// SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches); arguments of orc_search_by_bow.  valid1[i] == 0: the keyframe's slot is NULL
// (even i) or holds a bad MapPoint (odd i).  matches21[i2] = keyframe index of vpMapPointMatches[i2] or -1.
int os1_search_by_bow(const uint8_t* desc1, const float* angle1, const uint8_t* valid1, int n1, const uint32_t* fv1_nodes,
                      const uint32_t* fv1_off, const uint32_t* fv1_feat, int nfv1, const uint8_t* desc2, const float* angle2, int n2,
                      const uint32_t* fv2_nodes, const uint32_t* fv2_off, const uint32_t* fv2_feat, int nfv2, float nnratio,
                      int checkOri, int32_t* matches21) {
  KeyFrame kf;
  Frame F;
  std::vector<MapPoint> mp(n1);
  kf.N = n1; kf.mvKeysUn.resize(n1); kf.mDescriptors = descRows(desc1, n1); kf.mvpMapPoints.assign(n1, static_cast<MapPoint*>(NULL));
  for (int i = 0; i < n1; i++) {
    kf.mvKeysUn[i].angle = angle1[i];
    mp[i].id = i;
    mp[i].mbBad = !valid1[i];
    if (valid1[i] || (i & 1)) kf.mvpMapPoints[i] = &mp[i];
  }
  kf.mvKeys = kf.mvKeysUn;
  kf.mFeatVec = featVec(fv1_nodes, fv1_off, fv1_feat, nfv1);
  F.N = n2; F.mvKeys.resize(n2); F.mDescriptors = descRows(desc2, n2);
  for (int i = 0; i < n2; i++) F.mvKeys[i].angle = angle2[i];
  F.mvKeysUn = F.mvKeys;
  F.mFeatVec = featVec(fv2_nodes, fv2_off, fv2_feat, nfv2);
  std::vector<MapPoint*> out;
  ORBmatcher matcher(nnratio, checkOri != 0);
  const int r = matcher.SearchByBoW(&kf, F, out);
  ids(out, matches21);
  return r;
}

// SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12); arguments of orc_search_by_bow_kf.  matches12[i1] = index in keyframe 2 or -1.
int os1_search_by_bow_kf(const uint8_t* desc1, const float* angle1, const uint8_t* valid1, int n1, const uint32_t* fv1_nodes,
                         const uint32_t* fv1_off, const uint32_t* fv1_feat, int nfv1, const uint8_t* desc2, const float* angle2,
                         const uint8_t* valid2, int n2, const uint32_t* fv2_nodes, const uint32_t* fv2_off, const uint32_t* fv2_feat,
                         int nfv2, float nnratio, int checkOri, int32_t* matches12) {
  KeyFrame kf[2];
  std::vector<MapPoint> mp[2];
  const uint8_t* desc[2] = {desc1, desc2};
  const float* angle[2] = {angle1, angle2};
  const uint8_t* valid[2] = {valid1, valid2};
  const int n[2] = {n1, n2};
  for (int s = 0; s < 2; s++) {
    mp[s].resize(n[s]);
    kf[s].N = n[s]; kf[s].mvKeysUn.resize(n[s]); kf[s].mDescriptors = descRows(desc[s], n[s]);
    kf[s].mvpMapPoints.assign(n[s], static_cast<MapPoint*>(NULL));
    for (int i = 0; i < n[s]; i++) {
      kf[s].mvKeysUn[i].angle = angle[s][i];
      mp[s][i].id = i;
      mp[s][i].mbBad = !valid[s][i];
      if (valid[s][i] || (i & 1)) kf[s].mvpMapPoints[i] = &mp[s][i];
    }
    kf[s].mvKeys = kf[s].mvKeysUn;
  }
  kf[0].mFeatVec = featVec(fv1_nodes, fv1_off, fv1_feat, nfv1);
  kf[1].mFeatVec = featVec(fv2_nodes, fv2_off, fv2_feat, nfv2);
  std::vector<MapPoint*> out;
  ORBmatcher matcher(nnratio, checkOri != 0);
  const int r = matcher.SearchByBoW(&kf[0], &kf[1], out);
  ids(out, matches12);
  return r;
}

// SearchForTriangulation; arguments of orc_search_for_triangulation.  The reference computes the epipole from the two poses
// (ORBmatcher.cc:659-665): keyframe 2 gets the identity pose and fx = fy = 1, cx = cy = 0, keyframe 1 the camera centre
// (ex, ey, 1), for which C2 = R2w*Cw + t2w, 1/z and fx*C2.x*invz + cx reproduce (ex, ey) without a rounding.  pairs: n1 x 2.
int os1_search_for_triangulation(const OrcKp* kps1, const uint8_t* desc1, const uint8_t* hasMP1, int n1, const uint32_t* fv1_nodes,
                                 const uint32_t* fv1_off, const uint32_t* fv1_feat, int nfv1, const OrcKp* kps2, const uint8_t* desc2,
                                 const uint8_t* hasMP2, int n2, const uint32_t* fv2_nodes, const uint32_t* fv2_off,
                                 const uint32_t* fv2_feat, int nfv2, const float* F12, float ex, float ey, const float* scale2,
                                 const float* sigma2, int checkOri, int32_t* pairs) {
  KeyFrame k1, k2;
  MapPoint holder;
  k1.N = n1; k1.mvKeysUn = keys(kps1, n1); k1.mvKeys = k1.mvKeysUn; k1.mDescriptors = descRows(desc1, n1);
  k2.N = n2; k2.mvKeysUn = keys(kps2, n2); k2.mvKeys = k2.mvKeysUn; k2.mDescriptors = descRows(desc2, n2);
  k1.mvpMapPoints.assign(n1, static_cast<MapPoint*>(NULL));
  k2.mvpMapPoints.assign(n2, static_cast<MapPoint*>(NULL));
  for (int i = 0; i < n1; i++) if (hasMP1[i]) k1.mvpMapPoints[i] = &holder;
  for (int i = 0; i < n2; i++) if (hasMP2[i]) k2.mvpMapPoints[i] = &holder;
  k1.mFeatVec = featVec(fv1_nodes, fv1_off, fv1_feat, nfv1);
  k2.mFeatVec = featVec(fv2_nodes, fv2_off, fv2_feat, nfv2);
  int nlev = 1;
  for (int i = 0; i < n2; i++) nlev = std::max(nlev, kps2[i].octave + 1);
  k2.mvScaleFactors.assign(scale2, scale2 + nlev);
  k2.mvLevelSigma2.assign(sigma2, sigma2 + nlev);
  k2.fx = k2.fy = 1.f; k2.cx = k2.cy = 0.f;
  k2.SetPose(identity4());
  k1.SetPose(identity4());
  const float c[3] = {ex, ey, 1.f};
  k1.SetCameraCenter(cv::Mat(3, 1, CV_32F, c));
  std::vector<std::pair<size_t, size_t> > vp;
  ORBmatcher matcher(0.6f, checkOri != 0);
  const int r = matcher.SearchForTriangulation(&k1, &k2, cv::Mat(3, 3, CV_32F, F12), vp);
  for (size_t i = 0; i < vp.size(); i++) { pairs[2 * i] = (int32_t)vp[i].first; pairs[2 * i + 1] = (int32_t)vp[i].second; }
  return r;
}

// ---- the pose-driven members; arguments of oracle/orb_oracle_pose.h ----------------------------------------------------------
int os1_sbp_frame(const OrcView* cur, const float Tcw[16], const OrcKp* lastKeys, const OrcKp* lastKeysUn, int nLast,
                  const int32_t* last_mp, const uint8_t* last_outlier, OrcPoints* P, int32_t* cur_mp, float th, int check_orientation) {
  Table T(P, NULL);
  Frame Cur, Last;
  fillView(Cur, cur);
  Cur.mTcw = cv::Mat(4, 4, CV_32F, Tcw);
  Cur.mvpMapPoints = T.list(cur_mp, cur->n);
  Last.N = nLast; Last.mvKeys = keys(lastKeys, nLast); Last.mvKeysUn = keys(lastKeysUn, nLast);
  Last.mvpMapPoints = T.list(last_mp, nLast);
  Last.mvbOutlier.resize(nLast);
  for (int i = 0; i < nLast; i++) Last.mvbOutlier[i] = last_outlier[i] != 0;
  Last.mTcw = identity4();   // (read for tlc, which nothing uses)
  ORBmatcher matcher(0.9f, check_orientation != 0);
  const int r = matcher.SearchByProjection(Cur, Last, th);
  ids(Cur.mvpMapPoints, cur_mp);
  return r;
}

int os1_sbp_keyframe(const OrcView* cur, const float Tcw[16], const OrcKp* kfKeysUn, int nKF, const int32_t* kf_mp,
                     const uint8_t* already, OrcPoints* P, int32_t* cur_mp, float th, int ORBdist, int check_orientation) {
  Table T(P, NULL);
  Frame Cur;
  KeyFrame kf;
  fillView(Cur, cur);
  Cur.mTcw = cv::Mat(4, 4, CV_32F, Tcw);
  Cur.mvpMapPoints = T.list(cur_mp, cur->n);
  kf.N = nKF; kf.mvKeysUn = keys(kfKeysUn, nKF); kf.mvKeys = kf.mvKeysUn;
  kf.mvpMapPoints = T.list(kf_mp, nKF);
  std::set<MapPoint*> found;
  for (int i = 0; i < P->M; i++) if (already[i]) found.insert(T.at(i));
  ORBmatcher matcher(0.9f, check_orientation != 0);
  const int r = matcher.SearchByProjection(Cur, &kf, found, th, ORBdist);
  ids(Cur.mvpMapPoints, cur_mp);
  return r;
}

int os1_sbp_scw(const OrcView* kfv, const float Scw[16], const int32_t* points, int npoints, OrcPoints* P, int32_t* vpMatched, int th) {
  KeyFrame kf;
  Table T(P, &kf);
  fillView(kf, kfv);
  std::vector<MapPoint*> matched = T.list(vpMatched, kfv->n);
  ORBmatcher matcher(0.75f, true);
  const int r = matcher.SearchByProjection(&kf, cv::Mat(4, 4, CV_32F, Scw), T.list(points, npoints), matched, th);
  ids(matched, vpMatched);
  return r;
}

int os1_fuse(const OrcView* kfv, const float Tcw[16], const int32_t* cand, int ncand, OrcPoints* P, int32_t* slot, float th) {
  KeyFrame kf;
  Table T(P, &kf);
  fillView(kf, kfv);
  kf.SetPose(cv::Mat(4, 4, CV_32F, Tcw));
  kf.mvpMapPoints = T.list(slot, kfv->n);
  ORBmatcher matcher;
  const int r = matcher.Fuse(&kf, T.list(cand, ncand), th);
  ids(kf.mvpMapPoints, slot);
  return r;
}

int os1_fuse_scw(const OrcView* kfv, const float Scw[16], const int32_t* points, int npoints, OrcPoints* P, int32_t* slot, float th,
                 int32_t* replace_out) {
  KeyFrame kf;
  Table T(P, &kf);
  fillView(kf, kfv);
  kf.mvpMapPoints = T.list(slot, kfv->n);
  std::vector<MapPoint*> rep = T.list(replace_out, npoints);
  ORBmatcher matcher(0.8f);
  const int r = matcher.Fuse(&kf, cv::Mat(4, 4, CV_32F, Scw), T.list(points, npoints), th, rep);
  ids(kf.mvpMapPoints, slot);
  ids(rep, replace_out);
  return r;
}

int os1_search_by_sim3(const OrcView* kf1v, const float T1w[16], const int32_t* mp1, const OrcView* kf2v, const float T2w[16],
                       const int32_t* mp2, OrcPoints* P, int32_t* matches12, float s12, const float R12[9], const float t12[3], float th) {
  KeyFrame kf1, kf2;
  Table T(P, &kf2);   // idxInKF is GetIndexInKeyFrame(pKF2)
  fillView(kf1, kf1v);
  fillView(kf2, kf2v);
  kf1.SetPose(cv::Mat(4, 4, CV_32F, T1w));
  kf2.SetPose(cv::Mat(4, 4, CV_32F, T2w));
  kf1.mvpMapPoints = T.list(mp1, kf1v->n);
  kf2.mvpMapPoints = T.list(mp2, kf2v->n);
  std::vector<MapPoint*> m12 = T.list(matches12, kf1v->n);
  ORBmatcher matcher(0.75f, true);
  const int r = matcher.SearchBySim3(&kf1, &kf2, m12, s12, cv::Mat(3, 3, CV_32F, R12), cv::Mat(3, 1, CV_32F, t12), th);
  ids(m12, matches12);
  return r;
}

// the stand-in's arithmetic ALONE, for the test that holds it to the oracle's orc_cv_small: op 0 A*b+c (c may be NULL: A*b),
// 1 -A.t()*b, 2 cv::norm(b), 3 a.dot(b) on the first row of A, 4 -A*b, 5 s*A (9 out), 6 (1.0/s)*A.t() (9 out), 7 A/s (9 out),
// 8 b - c (3 out), 9 KeyFrame::SetPose's camera centre of [A | b]
void os1_cv_small(int op, const float* A, const float* b, const float* c, float s, float* out, double* out1) {
  const cv::Mat mA(3, 3, CV_32F, A);
  cv::Mat mb, mc, r;
  if (b) mb = cv::Mat(3, 1, CV_32F, b);
  if (c) mc = cv::Mat(3, 1, CV_32F, c);
  switch (op) {
    case 0: if (c) r = mA * mb + mc; else r = mA * mb; break;
    case 1: r = -mA.t() * mb; break;
    case 2: *out1 = cv::norm(mb); return;
    case 3: *out1 = mA.row(0).dot(mb); return;
    case 4: r = -mA * mb; break;
    case 5: r = s * mA; break;
    case 6: r = (1.0 / s) * mA.t(); break;
    case 7: r = mA / s; break;
    case 8: r = mb - mc; break;
    default: {
      cv::Mat T = identity4();
      for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T.at<float>(i, j) = A[3 * i + j]; T.at<float>(i, 3) = b[i]; }
      KeyFrame kf;
      kf.SetPose(T);
      r = kf.GetCameraCenter();
    }
  }
  for (int i = 0; i < r.rows * r.cols; i++) out[i] = r.at<float>(i);
}

}  // extern "C"
