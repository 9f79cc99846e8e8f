// include/orbfe/KeyFrameCulling.h through the C ABI on the GPU: orbfe::KeyFrameCulling on the stub maps of
// keyframe_culling_scenes.h, against the sequential loop on a second copy of each map.  Built and run by
// tests/test_gpu_keyframe_culling.py against liborbfe.so.
#include "keyframe_culling_scenes.h"

using namespace culling_scenes;

int main() {
  orbfe_matcher* m = nullptr;
  if (orbfe_matcher_create(0, &m) != ORBFE_OK) { std::printf("FAIL orbfe_matcher_create: %s\n", orbfe_last_error()); return 1; }
  auto run = [m](const std::vector<KeyFrame*>& v, orbfe::KeyFrameCullingStats* st) { return orbfe::KeyFrameCulling(m, v, st); };
  const int bad = all(run);
  orbfe_matcher_destroy(m);
  if (bad) return 1;
  std::printf("PASS\n");
  return 0;
}
