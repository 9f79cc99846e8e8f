// orbfe_window.hip -- the window kernel: Frame::GetFeaturesInArea (src/Frame.cc:209-262) over the 64x48 grid for every query of
// a call, with ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1605-1621) for every candidate, in the reference's candidate
// order.  One host entry, orbfe::launch_window_match, for its two callers: the host-array search (orbfe_matcher.hip) and the
// search on a resident frame (orbfe_frame.hip).  Parameter block and record format: orbfe_matcher_internal.h; the launch
// width: window_plan.h.
#include "orbfe_matcher_internal.h"

namespace orbfe_match {

// Outcome of a query restricted to the candidates whose bit is set in `avail`: 0 = no match, c + 1 = candidate c.
// mode 0: ORBmatcher::SearchByProjection(Frame&, MapPoints, th), src/ORBmatcher.cc:95-120 -- best / second best with their
// levels, TH_HIGH, the ratio test only when both lie on the same level; modes 1, 2: best <= maxDist (:1373-1383, :376-392).
// Entries: index | distance << 16 | octave << 25.
template <int NC>
__device__ __forceinline__ int outcome_of(int mode, int cnt, const uint32_t e[NC], unsigned avail, float nnratio, int maxDist) {
  int bestDist = mode == 2 ? INT_MAX : 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, best = -1;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (c >= cnt || !((avail >> c) & 1u)) continue;
    const int dist = (int)((e[c] >> 16) & 0x1ff), oct = (int)(e[c] >> 25);
    if (mode == 0) {
      if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = oct; best = c; }
      else if (dist < bestDist2) { bestLevel2 = oct; bestDist2 = dist; }
    } else if (dist < bestDist) {
      bestDist = dist; best = c;
    }
  }
  if (mode == 0) {
    if (bestDist > TH_HIGH) return 0;
    if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) return 0;
  } else if (bestDist > maxDist) {
    return 0;
  }
  return best + 1;
}

// LPQ lanes per query (64/LPQ queries per wave), one LANE per grid column of the window.  Window
// semantics: Frame::GetFeaturesInArea, Frame.cc:209-262: columns ix ascending, rows iy ascending inside a
// column, insertion order inside a cell -- i.e. for column ix the contiguous run
// [cellStart[ix*48+cy0], cellStart[ix*48+cy1+1]) of the cell-sorted keypoint table.  Lane l of a query's
// group walks the run of column cx0+l (a handful of entries), a prefix sum over the group's hit counts
// gives every lane its output offset, so the candidate list comes out in exactly the reference order in
// a single pass with all columns in flight at once.  The host picks LPQ >= the widest window in columns.
// A block is 4 waves (kWinThreads / LPQ queries); the pool space of ALL its queries is claimed with ONE atomic: ten thousand
// same-address atomics with return (one per query) serialise in the L2 and took longer than the search itself.
constexpr int kTmpEntries = 6;   // lists gathered in LDS: those of the record, and the lists of four to six candidates for their wide record
template <int LPQ>
__global__ __launch_bounds__(kWinThreads) void k_window_match(MatchParams M) {
  __shared__ uint32_t wtot[kWinThreads / 64];
  __shared__ uint32_t blockBase, blockBaseW;
  __shared__ uint32_t recTmp[(kWinThreads / LPQ) * kTmpEntries];   // short lists gathered per query (resident-frame searches)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (LPQ - 1);
  const int q = blockIdx.x * (kWinThreads / LPQ) + threadIdx.x / LPQ;
  const bool live = q < M.nq;
#pragma unroll
  for (int c = 0; c < 2; c++)
    for (int g0 = blockIdx.x * kWinThreads + wave * 64; g0 < M.bitN[c]; g0 += gridDim.x * kWinThreads) {
      const int g = g0 + lane;
      const unsigned long long bits =
          M.bitConst[c] >= 0 ? (M.bitConst[c] ? ~0ull : 0ull) : __ballot(g < M.bitN[c] && (M.bitSrc[c][g] & M.bitMask[c]) != 0);
      if (lane == 0) M.bitDst[c][g0 >> 6] = bits;
    }
  float r = -1.f, x = 0.f, y = 0.f;
  int minL = 0, maxL = -1;
  PairInfo pi = M.pairs[0];
  int drow = 0;   // row of the query's descriptor in an indexed table: requested together with the other query fields
  if (live && M.qdescRow) drow = M.qdescRow[q];
  if (live && M.rawKind) {
    const float2 p = reinterpret_cast<const float2*>(M.rawXY)[q];
    const int lvl = M.rawLevel[q];
    const unsigned fl = M.rawFlags[q];
    x = p.x; y = p.y;
    minL = lvl - 1;
    if (M.rawKind == 1) {
      maxL = lvl;                                      // GetFeaturesInArea(x, y, r * scale, nPredictedLevel - 1, nPredictedLevel)
      float rr = (fl & ORBFE_MP_CANDIDATO) ? 4.0f : ((double)M.rawAux[q] > 0.998 ? 2.5f : 4.0f);   // RadiusByViewingCos
      if (M.rawFactor) rr *= M.rawTh;
      r = ((fl & ORBFE_MP_IN_VIEW) && !(fl & ORBFE_MP_BAD)) ? rr * M.rawSf[lvl & 31] : -1.f;
    } else if (M.rawKind == 2) {
      maxL = lvl + 1;                                  // GetFeaturesInArea(u, v, radius, nLastOctave - 1, nLastOctave + 1)
      r = fl ? M.rawTh * M.rawSf[lvl & 31] : -1.f;
    } else {
      maxL = lvl;
      r = (fl && lvl >= 0) ? M.rawAux[q] : -1.f;       // no octave lies in [level - 1, level] for level < 0
    }
  } else if (live) {
    r = M.qr[q]; x = M.qx[q]; y = M.qy[q]; minL = M.qminL[q]; maxL = M.qmaxL[q];
    pi = M.pairs[M.qpair ? M.qpair[q] : 0];   // qpair == nullptr: every query searches pair 0 (a resident frame)
  }
  const float* sx = M.sx + pi.trainOff;
  const float* sy = M.sy + pi.trainOff;
  const int* soct = M.soct + pi.trainOff;
  const int* sidx = M.sidx + pi.trainOff;
  const int* cellStart = M.cellStart + pi.cellOff;
  const uint8_t* tdesc = M.tdesc + (size_t)pi.tdescOff * 32;
  int cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1;
  if (live && r >= 0.f) {
    cx0 = max(0, (int)floorf((x - pi.minX - r) * pi.invW));
    cx1 = min(kGridCols - 1, (int)ceilf((x - pi.minX + r) * pi.invW));
    cy0 = max(0, (int)floorf((y - pi.minY - r) * pi.invH));
    cy1 = min(kGridRows - 1, (int)ceilf((y - pi.minY + r) * pi.invH));
    if (cx0 >= kGridCols || cx1 < 0 || cy0 >= kGridRows || cy1 < 0) cx1 = cx0 - 1;  // empty window
  }
  // the query's descriptor is fetched now, with the window still unknown: it may come over PCIe (page-locked rows read in
  // place), and that round trip then overlaps the walk of the grid instead of following it
  uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live && r >= 0.f) {
    const uint4* qp = reinterpret_cast<const uint4*>(M.qdesc + (size_t)q * 32);
    if (M.qdescRow) {
      const unsigned row = (unsigned)drow;
      qp = reinterpret_cast<const uint4*>(((row >> 31) ? M.qdescAlt : M.qdesc) + (size_t)(row & 0x7fffffffu) * 32);
    }
    const uint4 a = qp[0], b4 = qp[1];
    qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b4.x; qd[5] = b4.y; qd[6] = b4.z; qd[7] = b4.w;
  }
  const bool checkLevels = (minL > 0) || (maxL >= 0);
  const int ix = cx0 + sub;
  int b = 0, e1 = 0;
  if (ix <= cx1) {
    b = cellStart[ix * kGridRows + cy0];
    e1 = cellStart[ix * kGridRows + cy1 + 1];
  }
  auto inWindow = [&](int e) -> bool {
    if (checkLevels) {
      const int o = soct[e];
      if (o < minL) return false;
      if (maxL >= 0 && o > maxL) return false;
    }
    const float dx = sx[e] - x, dy = sy[e] - y;
    if (!(fabsf(dx) < r && fabsf(dy) < r)) return false;
    if (M.invSigma2) {   // (u - kp.x)^2 + (v - kp.y)^2: a float difference and its negation have the same square
      const float e2 = dx * dx + dy * dy;
      if ((double)(e2 * M.invSigma2[soct[e]]) > M.chi2) return false;
    }
    return true;
  };
  // pass 1: hits per column (the first 64 entries of a run remember their verdict in a bit mask, so the second pass
  // does not fetch their coordinates again), prefix sum inside the query's lane group.  The run is walked four entries at
  // a time with all their loads issued before the first test: a lane's run is a handful of entries, and one dependent
  // memory round trip per ENTRY (what a plain loop costs) was the kernel's whole duration.
  int hits = 0;
  unsigned long long hm = 0;
  for (int e = b; e < e1; e += 4) {
    float kx[4], ky[4];
    int ko[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int ee = min(e + u, e1 - 1);
      kx[u] = sx[ee]; ky[u] = sy[ee]; ko[u] = soct[ee];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (e + u >= e1) break;
      bool h = true;
      if (checkLevels) h = !(ko[u] < minL) && !(maxL >= 0 && ko[u] > maxL);
      const float dx = kx[u] - x, dy = ky[u] - y;
      h = h && fabsf(dx) < r && fabsf(dy) < r;
      if (h && M.invSigma2) {   // (u - kp.x)^2 + (v - kp.y)^2: a float difference and its negation have the same square
        const float e2 = dx * dx + dy * dy;
        if ((double)(e2 * M.invSigma2[ko[u]]) > M.chi2) h = false;
      }
      hits += h ? 1 : 0;
      if (h && e + u - b < 64) hm |= 1ull << (e + u - b);
    }
  }
  // pass 1b (searches on a resident frame): candidates whose distance rules them out whatever the other queries do never
  // enter the list -- shorter lists mean records instead of walked lists and fewer rounds of the bookkeeping, with the
  // same outcome.  Modes 1, 2 (best <= maxDist decides alone, ORBmatcher.cc:1373-1383, :376-392): dist > maxDist.  Mode 0
  // (:95-120): a candidate with dist > TH_HIGH and nnratio * dist >= TH_HIGH can neither be accepted nor, as second best, make
  // the ratio test reject an acceptable best (bestDist <= TH_HIGH <= nnratio * dist); dropping it leaves, in its place, a
  // second best that is at least as far, i.e. as irrelevant.  Distances are computed here for the verdict only; the
  // survivors' entries are produced by pass 2 as before.  Runs beyond the 64-entry mask are left as they are.
  const uint4* td4 = reinterpret_cast<const uint4*>(tdesc);   // descriptors are grid-sorted, 32-byte rows
  if (M.rec && hm) {
    unsigned long long left = hm;
    while (left) {
      const int a0 = __builtin_ctzll(left);
      left &= left - 1;
      const int a1 = left ? __builtin_ctzll(left) : a0;
      left &= left - 1;   // (no-op when a1 == a0 was the last bit: left is 0)
      const uint4 da0 = td4[(size_t)(b + a0) * 2], da1 = td4[(size_t)(b + a0) * 2 + 1], db0 = td4[(size_t)(b + a1) * 2],
                  db1 = td4[(size_t)(b + a1) * 2 + 1];
      const int d0 = __popc(da0.x ^ qd[0]) + __popc(da0.y ^ qd[1]) + __popc(da0.z ^ qd[2]) + __popc(da0.w ^ qd[3]) + __popc(da1.x ^ qd[4]) +
                     __popc(da1.y ^ qd[5]) + __popc(da1.z ^ qd[6]) + __popc(da1.w ^ qd[7]);
      const int d1 = __popc(db0.x ^ qd[0]) + __popc(db0.y ^ qd[1]) + __popc(db0.z ^ qd[2]) + __popc(db0.w ^ qd[3]) + __popc(db1.x ^ qd[4]) +
                     __popc(db1.y ^ qd[5]) + __popc(db1.z ^ qd[6]) + __popc(db1.w ^ qd[7]);
      // (d > TH_HIGH spelled out: for nnratio >= 1 the product alone would drop an acceptable candidate, e.g. d == 100)
      const bool drop0 = M.codeMode == 0 ? (d0 > TH_HIGH && M.nnratio * (float)d0 >= (float)TH_HIGH) : d0 > M.maxDist;
      const bool drop1 = M.codeMode == 0 ? (d1 > TH_HIGH && M.nnratio * (float)d1 >= (float)TH_HIGH) : d1 > M.maxDist;
      if (drop0) { hm &= ~(1ull << a0); hits--; }
      if (drop1 && a1 != a0) { hm &= ~(1ull << a1); hits--; }
    }
  }
  int incl = hits;
#pragma unroll
  for (int o = 1; o < LPQ; o <<= 1) {
    const int t = __shfl_up(incl, o, LPQ);
    if (sub >= o) incl += t;
  }
  const uint32_t count = (uint32_t)__shfl(incl, LPQ - 1, LPQ);
  // a resident-frame search keeps lists of up to kRecEntries candidates in the query's fixed 16-byte record (no pool space,
  // no offset to chase); longer lists go to the pool like every list of the host-resolved searches
  const bool inRec = M.rec != nullptr && count <= (uint32_t)kRecEntries;
  const bool wide = M.rec != nullptr && count >= 4u && count <= (uint32_t)kWideMax;   // entries to the pool AND (via LDS) a wide record
  // offsets: exclusive scan of the queries' counts inside the wave, of the wave totals inside the block, one atomic per pool.
  // Both sums travel in one word: pool entries in the low 24 bits, wide-record words in the high 8 (a wave has at most
  // eight queries: 8 x 65 535 entries, 8 x 11 words).
  const uint32_t mine = (live && sub == 0 && !inRec) ? (count | (wide ? wide_words(count) << 24 : 0u)) : 0u;
  uint32_t wincl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(wincl, o, 64);
    if (lane >= o) wincl += t;
  }
  if (lane == 63) wtot[wave] = wincl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0, sw = 0;
    for (int w = 0; w < kWinThreads / 64; w++) { s += wtot[w] & 0xffffffu; sw += wtot[w] >> 24; }
    blockBase = s ? atomicAdd(M.total, s) : 0u;
    blockBaseW = sw ? atomicAdd(M.wtotal, sw) : 0u;
  }
  __syncthreads();
  uint32_t off = blockBase + ((wincl - mine) & 0xffffffu), offW = blockBaseW + ((wincl - mine) >> 24);
  for (int w = 0; w < wave; w++) { off += wtot[w] & 0xffffffu; offW += wtot[w] >> 24; }
  if (live && sub == 0) {
    M.qcount[q] = count;
    M.qoff[q] = off;
  }
  off = __shfl(off, 0, LPQ);
  if (hits == 0 && !M.rec) return;
  const int qlocal = threadIdx.x / LPQ;
  // pass 2: distances, written at the lane's position in column order; the hits of the mask are fetched two at a time
  uint32_t pos = (uint32_t)(incl - hits);   // position inside the query's list
  auto emit = [&](int e, int idx, int oct, const uint4& d0, const uint4& d1) {
    const int d = __popc(d0.x ^ qd[0]) + __popc(d0.y ^ qd[1]) + __popc(d0.z ^ qd[2]) + __popc(d0.w ^ qd[3]) + __popc(d1.x ^ qd[4]) +
                  __popc(d1.y ^ qd[5]) + __popc(d1.z ^ qd[6]) + __popc(d1.w ^ qd[7]);
    uint32_t entry = (uint32_t)idx | ((uint32_t)d << 16);
    if (M.packOctave) entry |= (uint32_t)oct << 25;
    if (inRec || wide) recTmp[qlocal * kTmpEntries + pos] = entry;
    if (!inRec && off + pos < M.poolCap) M.pool[off + pos] = entry;
    pos++;
  };
  while (hm) {
    const int a0 = __builtin_ctzll(hm);
    hm &= hm - 1;
    const int a1 = hm ? __builtin_ctzll(hm) : a0;
    const bool two = hm != 0;
    if (two) hm &= hm - 1;
    const int ea = b + a0, eb = b + a1;
    const int ia = sidx[ea], ib = sidx[eb], oa = soct[ea], ob = soct[eb];
    const uint4 da0 = td4[(size_t)ea * 2], da1 = td4[(size_t)ea * 2 + 1], db0 = td4[(size_t)eb * 2], db1 = td4[(size_t)eb * 2 + 1];
    emit(ea, ia, oa, da0, da1);
    if (two) emit(eb, ib, ob, db0, db1);
  }
  for (int e = b + 64; e < e1; e++) {   // runs beyond the mask (very wide windows)
    if (!inWindow(e)) continue;
    emit(e, sidx[e], soct[e], td4[(size_t)e * 2], td4[(size_t)e * 2 + 1]);
  }
  if (M.rec) {
    // the query's record: its lanes' entries meet in LDS (a query's lanes are one wave's: a wave-level fence is enough).
    // The outcomes are tabulated by the group's first eight lanes, ONE availability pattern each (one per code word for a
    // wide record), and OR-ed together by three shuffles; lane 0 writes the 16 bytes at once.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (live && inRec) {
      uint32_t e3[3];
#pragma unroll
      for (int c = 0; c < 3; c++) e3[c] = (uint32_t)c < count ? recTmp[qlocal * kTmpEntries + c] : 0u;
      const unsigned p = (unsigned)sub & 7u;
      uint32_t code = 0u;
      if (sub < 8 && p) code = (uint32_t)outcome_of<3>(M.codeMode, (int)count, e3, p & ((1u << count) - 1u), M.nnratio, M.maxDist) << (2u * p);
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) code |= (uint32_t)__shfl_xor((int)code, o, LPQ);
      if (sub == 0) {
        reinterpret_cast<uint4*>(M.rec)[q] = make_uint4(count | (code << 16), e3[0], e3[1], e3[2]);
        if (M.qword) M.qword[q] = make_uint2((e3[0] & 0xffffu) | (e3[1] << 16), (e3[2] & 0xffffu) | (code << 16));
      }
    } else if (live && wide) {
      uint32_t e6[kWideMax];
#pragma unroll
      for (int c = 0; c < kWideMax; c++) e6[c] = (uint32_t)c < count ? recTmp[qlocal * kTmpEntries + c] : 0u;
      const unsigned p = (unsigned)sub & 7u;
      const int nW = 1 << ((int)count - 3);     // code words: 2, 4, 8
      uint32_t* wr = M.wpool + offW;
#pragma unroll
      for (int w = 0; w < 8; w++) {
        if (w >= nW) break;                      // (uniform inside the group)
        uint32_t word = 0u;
        if (sub < 8 && (w | p)) word = (uint32_t)outcome_of<kWideMax>(M.codeMode, (int)count, e6, 8u * w + p, M.nnratio, M.maxDist) << (3u * p);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) word |= (uint32_t)__shfl_xor((int)word, o, LPQ);
        if (sub == 0) wr[3 + w] = word;
      }
      if (sub == 0) {
        wr[0] = (e6[0] & 0xffffu) | (e6[1] << 16);
        wr[1] = (e6[2] & 0xffffu) | (e6[3] << 16);
        wr[2] = (e6[4] & 0xffffu) | (e6[5] << 16);
        reinterpret_cast<uint4*>(M.rec)[q] = make_uint4(count | (kCodeWide << 16), 0u, 0u, 0u);
        if (M.qword) M.qword[q] = make_uint2(offW, count | (kCodeWide << 16));
      }
    } else if (live && sub == 0) {
      reinterpret_cast<uint4*>(M.rec)[q] = make_uint4(count | (kCodeLongList << 16), 0u, 0u, 0u);
      if (M.qword) M.qword[q] = make_uint2(off, count | (kCodeLongList << 16));
    }
  }
}

}  // namespace orbfe_match

// The one launch of the window kernel, on `st` of the current device.  widestCols: the call's widest window in grid columns
// (window_plan.h says what both callers pass, and which width selects which instantiation).
int orbfe::launch_window_match(const orbfe_match::MatchParams& M, float widestCols, hipStream_t st) {
  using namespace orbfe_match;
  const int lpq = window_lanes(widestCols);
  const dim3 grid(window_blocks((size_t)M.nq, lpq)), block(kWinThreads);
  if (lpq == 8) hipLaunchKernelGGL(k_window_match<8>, grid, block, 0, st, M);
  else if (lpq == 16) hipLaunchKernelGGL(k_window_match<16>, grid, block, 0, st, M);
  else if (lpq == 32) hipLaunchKernelGGL(k_window_match<32>, grid, block, 0, st, M);
  else hipLaunchKernelGGL(k_window_match<64>, grid, block, 0, st, M);
  HIP_TRY(hipGetLastError());
  return ORBFE_OK;
}
