// equidistant_facade_test.cpp -- orbfe::Extractor::SetEquidistantCamera through a Tracking-shaped sequence of a camaraModo == 1
// (equidistant fisheye) camera; every frame's mvKeysUn is also compared with the host orbfe::UndistortKeyPoints(.., 1, ..):
//   per frame   Frame::Frame: ExtractORB + UndistortKeyPoints (extractUndistorted) -> (grid)        Frame.cc:100-111
//               first search of the frame: MatcherContext::resident (the frame's features on the GPU), a second lookup
//   per pair    SearchForInitialization(previous, current) on mvKeysUn                               Tracking.cc:383-384
// It asserts that no frame's features were uploaded and that NOT ONE byte of undistorted coordinates was sent (the resident
// frames take them where the undistortion kernel left them), and writes what it computed for the Python driver, which holds
// the oracle: f<k>.un = mvKeysUn x, y as the resident frame holds them, f<k>.kp / .desc, p<k>.m12 / .nm per pair.
// usage: equidistant_facade_test DIR   (DIR/meta.txt: W H NF nfeat fx fy cx cy; DIR/f<k>.gray)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "orbfe/orb_shim.hpp"

struct KeyPoint { float x, y, size, angle, response; int octave, class_id; };
struct Point2f { float x, y; };
struct Mat {
  unsigned char* data = nullptr;
  size_t step = 0;
  int rows = 0;
};
struct Frame {
  std::vector<KeyPoint> mvKeys, mvKeysUn;
  std::vector<unsigned char> descStore;
  Mat mDescriptors;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
  void bind() { mDescriptors.data = descStore.data(); mDescriptors.step = 32; mDescriptors.rows = (int)mvKeys.size(); }
};
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

static std::vector<unsigned char> readFile(const std::string& p) {
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", p.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> v(n);
  if (fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}
static void writeFile(const std::string& p, const void* d, size_t n) {
  FILE* f = fopen(p.c_str(), "wb");
  if (!f || fwrite(d, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", p.c_str()); exit(2); }
  fclose(f);
}
static int failures = 0;
static void expect(bool ok, const char* what, long got) {
  if (!ok) { failures++; printf("FAIL: %s (got %ld)\n", what, got); }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  int W, H, NF, nfeat;
  float fx, fy, cx, cy;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%d %d %d %d %f %f %f %f", &W, &H, &NF, &nfeat, &fx, &fy, &cx, &cy) != 8) return 2;
    fclose(f);
  }
  const int device = orbfe::detail::defaultDevice();
  orbfe::Extractor extractor(nfeat, 1.2f, 8, 20, 7, device);
  bool refused = false;
  try { extractor.SetCamera(1, fx, fy, cx, cy, nullptr, 0); } catch (const std::exception&) { refused = true; }
  expect(refused, "SetCamera(1, ..) was not refused", 0);
  extractor.SetEquidistantCamera(fx, fy, cx, cy);
  orbfe::MatcherContext ctx(device);
  orbfe::ComputeImageBounds(W, H, 1, fx, fy, cx, cy, nullptr, 0, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY);
  Frame last;
  for (int k = 0; k < NF; k++) {
    std::vector<unsigned char> img = readFile(dir + "/f" + std::to_string(k) + ".gray");
    Frame cur;
    extractor.extractUndistorted(img.data(), H, W, (size_t)W, cur.mvKeys, &cur.mvKeysUn, cur.descStore);   // ExtractORB + UndistortKeyPoints
    cur.bind();
    const int n = (int)cur.mvKeys.size();
    std::vector<KeyPoint> hostUn;
    orbfe::UndistortKeyPoints(cur.mvKeys, hostUn, 1, fx, fy, cx, cy, nullptr, 0);   // Frame::UndistortKeyPoints on the host
    expect(hostUn.size() == cur.mvKeysUn.size() && (n == 0 || !memcmp(hostUn.data(), cur.mvKeysUn.data(), (size_t)n * sizeof(KeyPoint))),
           "extractUndistorted differs from the host UndistortKeyPoints", k);
    orbfe_frame* fr = ctx.resident(cur, 0);          // the frame's first search
    expect(fr != nullptr && orbfe_frame_size(fr) == n, "no resident frame", n);
    expect(ctx.resident(cur, 0) == fr, "the second lookup built another frame", k);
    std::vector<OrbfeKeyPoint> dk(n > 0 ? n : 1);
    orbfe::check(orbfe_frame_download(fr, dk.data(), nullptr, nullptr, nullptr));
    std::vector<float> un((size_t)n * 2);
    for (int i = 0; i < n; i++) { un[2 * i] = dk[i].x; un[2 * i + 1] = dk[i].y; }
    bool same = true;
    for (int i = 0; i < n; i++) same = same && dk[i].x == cur.mvKeysUn[i].x && dk[i].y == cur.mvKeysUn[i].y;
    expect(same, "the resident frame's coordinates are not the Frame's mvKeysUn", k);
    const std::string pre = dir + "/f" + std::to_string(k);
    writeFile(pre + ".un", un.data(), un.size() * 4);
    writeFile(pre + ".kp", cur.mvKeys.data(), (size_t)n * sizeof(KeyPoint));
    writeFile(pre + ".desc", cur.descStore.data(), (size_t)n * 32);
    if (k > 0) {
      std::vector<Point2f> prevMatched(last.mvKeysUn.size());
      for (size_t i = 0; i < prevMatched.size(); i++) prevMatched[i] = Point2f{last.mvKeysUn[i].x, last.mvKeysUn[i].y};   // Tracking.cc:355-357
      std::vector<int> m12;
      const int nm = orbfe::SearchForInitialization(ctx, 0.9f, true, last, cur, prevMatched, m12, 100);
      writeFile(dir + "/p" + std::to_string(k) + ".m12", m12.data(), m12.size() * 4);
      writeFile(dir + "/p" + std::to_string(k) + ".nm", &nm, 4);
    }
    last = cur;
    last.bind();
  }
  printf("uploads %zu from_extract %zu hits %zu coordinate_bytes %zu\n", ctx.residentUploads(), ctx.residentFromExtract(), ctx.residentHits(),
         ctx.residentCoordBytes());
  expect(ctx.residentUploads() == 0, "a frame's features were uploaded although the extractor held them", (long)ctx.residentUploads());
  expect(ctx.residentCoordBytes() == 0, "undistorted coordinates were sent although the arena held them", (long)ctx.residentCoordBytes());
  expect((int)ctx.residentFromExtract() == NF && (int)ctx.residentHits() == NF, "frames from the arena / cache hits", (long)ctx.residentFromExtract());
  printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
