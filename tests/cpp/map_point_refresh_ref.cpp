// An own restatement of MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:227-292) and
// MapPoint::UpdateNormalAndDepth (:315-356) over plain arrays, in the reference's own loop structure (a full N x N distance
// matrix, std::sort per row, the element at (size_t)(0.5*(N-1)), the first minimum; cv::Mat float arithmetic spelled out):
// the CPU yardstick of orbfe_local_map_refresh_rows.  Same arguments as that call, with a host table of 64-byte rows and, per
// keyframe slot, the descriptor rows and octaves as host arrays.  Build with -ffp-contract=off.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

int descriptorDistance(const uint8_t* a, const uint8_t* b) {   // ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1605-1621)
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    uint32_t x, y;
    std::memcpy(&x, a + 4 * i, 4);
    std::memcpy(&y, b + 4 * i, 4);
    unsigned int v = x ^ y;
    v = v - ((v >> 1) & 0x55555555);
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
    dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
  }
  return dist;
}

float cvNorm3(const float v[3]) {   // cv::norm of a 3x1 CV_32F: the squares summed in double, in index order
  double s = 0.0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return (float)std::sqrt(s);
}

double cvNorm3d(const float v[3]) {
  double s = 0.0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return std::sqrt(s);
}

}  // namespace

extern "C" {

// Index inside `descs` ([N][32]) of the descriptor with the least median distance to the rest; -1 for N == 0.
int mpr_distinctive(const uint8_t* descs, int N) {
  if (N <= 0) return -1;
  std::vector<float> Distances((size_t)N * N);
  for (int i = 0; i < N; i++) {
    Distances[(size_t)i * N + i] = 0;
    for (int j = i + 1; j < N; j++) {
      const int distij = descriptorDistance(descs + 32 * (size_t)i, descs + 32 * (size_t)j);
      Distances[(size_t)i * N + j] = (float)distij;
      Distances[(size_t)j * N + i] = (float)distij;
    }
  }
  int BestMedian = INT_MAX, BestIdx = 0;
  for (int i = 0; i < N; i++) {
    std::vector<int> vDists(Distances.begin() + (size_t)i * N, Distances.begin() + (size_t)(i + 1) * N);
    std::sort(vDists.begin(), vDists.end());
    const int median = vDists[(size_t)(0.5 * (N - 1))];
    if (median < BestMedian) { BestMedian = median; BestIdx = i; }
  }
  return BestIdx;
}

// UpdateNormalAndDepth for one MapPoint: n observations' camera centres Ow [n][3] in order, the reference keyframe's centre and
// level scale, the last level's scale.  out = normal[3], mfMinDistance, mfMaxDistance.
void mpr_normal_depth(const float pos[3], int n, const float* Ow, const float OwRef[3], float levelScaleFactor, float lastScaleFactor,
                      float out[5]) {
  float normal[3] = {0.0f, 0.0f, 0.0f};                        // cv::Mat::zeros(3,1,CV_32F)
  for (int i = 0; i < n; i++) {
    float normali[3];
    for (int k = 0; k < 3; k++) normali[k] = pos[k] - Ow[3 * (size_t)i + k];
    const float beta = (float)(1.0 / cvNorm3d(normali));       // normali/cv::norm(normali): a scale by 1.0/norm, held as float
    for (int k = 0; k < 3; k++) {
      const float t = normali[k] * beta;                       // cv::scaleAdd: the product rounds, then the sum
      normal[k] = t + normal[k];
    }
  }
  float PC[3];
  for (int k = 0; k < 3; k++) PC[k] = pos[k] - OwRef[k];
  const float dist = cvNorm3(PC);
  const float maxD = dist * levelScaleFactor;
  const float minD = maxD / lastScaleFactor;
  const float inv = (float)(1.0 / (double)n);                  // normal/n: convertTo(alpha = 1.0/n, beta = 0)
  for (int k = 0; k < 3; k++) {
    const float t = normal[k] * inv;
    out[k] = t + 0.0f;
  }
  out[3] = minD;
  out[4] = maxD;
}

// The batch, as orbfe_local_map_refresh_rows: returns 0, or -1 - p for the first MapPoint p whose reference level lies outside
// [0, nlevels) (its row is left as it was, the others are written).
int mpr_refresh_rows(uint8_t* table, int what, int n_kf, const uint8_t* const* kf_desc, const int32_t* const* kf_oct, const float* kf_Ow,
                     const float* scale_factors, int nlevels, int n_mp, const int32_t* rows, const int32_t* obs_offsets,
                     const int32_t* obs_kf, const int32_t* obs_kp, const uint8_t* obs_flags, const int32_t* ref_kf, const int32_t* ref_kp,
                     int32_t* best_obs, float* normal, float* min_raw, float* max_raw) {
  (void)n_kf;
  int firstBad = 0;
  for (int p = 0; p < n_mp; p++) {
    float* row = reinterpret_cast<float*>(table + 64 * (size_t)rows[p]);
    const int a = obs_offsets[p], n = obs_offsets[p + 1] - a;
    int best = -1;
    bool skip = false;
    int level = 0;
    if ((what & 2) && n > 0) {
      level = kf_oct[ref_kf[p]][ref_kp[p]];
      if (level < 0 || level >= nlevels) {
        skip = true;
        if (!firstBad) firstBad = -1 - p;
      }
    }
    if (!skip && (what & 1) && n > 0) {
      std::vector<uint8_t> v;
      std::vector<int> at;
      for (int o = 0; o < n; o++) {
        if (obs_flags && (obs_flags[a + o] & 1)) continue;     // if(!pKF->isBad())
        const uint8_t* d = kf_desc[obs_kf[a + o]] + 32 * (size_t)obs_kp[a + o];
        v.insert(v.end(), d, d + 32);
        at.push_back(o);
      }
      const int b = mpr_distinctive(v.data(), (int)at.size());
      if (b >= 0) {
        best = at[b];
        std::memcpy(reinterpret_cast<uint8_t*>(row) + 32, v.data() + 32 * (size_t)b, 32);
      }
    }
    if (!skip && (what & 2) && n > 0) {
      std::vector<float> Ow(3 * (size_t)n);
      for (int o = 0; o < n; o++) std::memcpy(&Ow[3 * (size_t)o], kf_Ow + 3 * (size_t)obs_kf[a + o], 12);
      float out[5];
      mpr_normal_depth(row, n, Ow.data(), kf_Ow + 3 * (size_t)ref_kf[p], scale_factors[level], scale_factors[nlevels - 1], out);
      std::memcpy(row + 3, out, 20);
    }
    if (best_obs) best_obs[p] = best;
    if (normal) std::memcpy(normal + 3 * (size_t)p, row + 3, 12);
    if (min_raw) min_raw[p] = row[6];
    if (max_raw) max_raw[p] = row[7];
  }
  return firstBad;
}

}  // extern "C"
