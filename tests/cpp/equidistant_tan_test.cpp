// Host build of os1_amd/csrc/equidistant_tan.h for tests/test_equidistant_tan.py and tools/find_equidistant_undecided.py.
//
//   enc IN OUT                    IN: float64 thetas.  OUT: 8 float64 per theta: ok, hi, lo_l, hi_l, ncand, cand0, cand1, cand2
//   verdict fx fy cx cy IN OUT    IN: float32 (u, v) pairs.  OUT: 3 float32 per point: x, y, undecided (0 / 1)
//   scan fx fy cx cy x0 x1 y0 y1 seed count threads
//                                 uniform float32 points of [x0, x1) x [y0, y1): prints "u v" (hex floats) of every undecided
//                                 point, then "scanned N undecided M"
//   centres fx fy u v x0 x1 y0 y1 seed count threads
//                                 the same over principal points (cx, cy) of [x0, x1) x [y0, y1) for the fixed point (u, v): prints
//                                 "cx cy" of every centre that makes it undecided
// A stand-alone program: build it with -fsanitize=address,undefined and run it directly for a sanitizer pass.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "equidistant_tan.h"

using namespace orbfe;

template <class T> static std::vector<T> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)n / sizeof(T));
  if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
  fclose(f);
  return v;
}

template <class T> static void dump(const char* path, const std::vector<T>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); exit(2); }
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
  fclose(f);
}

static EquidistantCamera camera(char** a) {
  const float fx = strtof(a[0], nullptr), fy = strtof(a[1], nullptr), cx = strtof(a[2], nullptr), cy = strtof(a[3], nullptr);
  return {fx, fy, cx, cy};
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "enc")) {
    const std::vector<double> th = slurp<double>(argv[2]);
    std::vector<double> out(th.size() * 8, 0.0);
    for (size_t i = 0; i < th.size(); i++) {
      const TanEnclosure e = tan_enclosure(th[i]);
      double* o = &out[i * 8];
      o[0] = e.ok;
      if (!e.ok) continue;
      o[1] = e.hi; o[2] = e.lo_l; o[3] = e.hi_l;
      o[4] = tan_candidates(e, o + 5);
    }
    dump(argv[3], out);
    return 0;
  }
  if (argc == 8 && !strcmp(argv[1], "verdict")) {
    const EquidistantCamera C = camera(argv + 2);
    const std::vector<float> in = slurp<float>(argv[6]);
    std::vector<float> out(in.size() / 2 * 3);
    for (size_t i = 0; i < in.size() / 2; i++) {
      const bool decided = equidistant_verdict(C, in[2 * i], in[2 * i + 1], &out[3 * i], &out[3 * i + 1]);
      out[3 * i + 2] = decided ? 0.f : 1.f;
    }
    dump(argv[7], out);
    return 0;
  }
  const bool centres = argc == 13 && !strcmp(argv[1], "centres");
  if (centres || (argc == 13 && !strcmp(argv[1], "scan"))) {
    const EquidistantCamera C0 = camera(argv + 2);   // (centres: the last two are the point)
    const float x0 = strtof(argv[6], nullptr), x1 = strtof(argv[7], nullptr), y0 = strtof(argv[8], nullptr), y1 = strtof(argv[9], nullptr);
    const unsigned long long seed = strtoull(argv[10], nullptr, 10), count = strtoull(argv[11], nullptr, 10);
    const int nt = atoi(argv[12]);
    std::mutex mu;
    unsigned long long found = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++)
      pool.emplace_back([&, t] {
        std::mt19937_64 rng(seed * 1000003ull + (unsigned)t);
        std::uniform_real_distribution<float> dx(x0, x1), dy(y0, y1);
        for (unsigned long long i = (unsigned)t; i < count; i += (unsigned)nt) {
          const float a = dx(rng), b = dy(rng);
          const float u = centres ? (float)C0.cx : a, v = centres ? (float)C0.cy : b;
          const EquidistantCamera C = centres ? EquidistantCamera{C0.fx, C0.fy, a, b} : C0;
          // cheap superset first: the host tan is within 1 ULP of the real value and every candidate is too, so all candidates lie
          // within 2 ULP of it; only a point whose floats move over that range can be undecided
          const double pw0 = ((double)u - C.cx) / C.fx, pw1 = ((double)v - C.cy) / C.fy;
          const double th = std::sqrt(pw0 * pw0 + pw1 * pw1);
          if (th > kThetaMin && th <= kThetaMax) {
            const double tn = std::tan(th);
            float ax, ay, bx, by;
            equidistant_project(C, pw0, pw1, tn * (1 - 0x1p-50) / th, &ax, &ay);
            equidistant_project(C, pw0, pw1, tn * (1 + 0x1p-50) / th, &bx, &by);
            if (ax == bx && ay == by) continue;
          }
          float ox, oy;
          if (equidistant_verdict(C, u, v, &ox, &oy)) continue;
          std::lock_guard<std::mutex> lk(mu);
          found++;
          printf("%a %a\n", (double)a, (double)b);
        }
      });
    for (auto& th : pool) th.join();
    printf("scanned %llu undecided %llu\n", count, found);
    return 0;
  }
  fprintf(stderr, "usage: see the head of tests/cpp/equidistant_tan_test.cpp\n");
  return 2;
}
