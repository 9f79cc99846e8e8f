// include/orbfe/KeyFrameCulling.h on a CPU: orbfe::KeyFrameCullingWith with the restated counter (keyframe_culling_ref.cpp) on the
// stub maps of keyframe_culling_scenes.h, against the sequential loop on a second copy of each map.  Also: a counter that fails
// leaves every object as it was, in the first round and in a later one.  Built by tests/test_keyframe_culling.py, also with
// -fsanitize=address,undefined.
#include "keyframe_culling_scenes.h"

extern "C" const char* orbfe_last_error(void) { return "(host build)"; }

using namespace culling_scenes;

namespace {
int gCalls = 0, gFailAt = 0;
int failing(int n_kf, int n_mp, const int32_t* oo, const int32_t* ok, const uint8_t* ol, const int32_t* nobs, int n_subj, const int32_t* ss, const int32_t* so,
            const int32_t* sm, const uint8_t* sl, int th, int32_t* a, int32_t* b) {
  if (++gCalls == gFailAt) return ORBFE_ERR_HIP;
  return kfcull_ref_counts(n_kf, n_mp, oo, ok, ol, nobs, n_subj, ss, so, sm, sl, th, a, b);
}
}  // namespace

int main() {
  auto run = [](const std::vector<KeyFrame*>& v, orbfe::KeyFrameCullingStats* st) { return orbfe::KeyFrameCullingWith(kfcull_ref_counts, v, st); };
  if (all(run)) return 1;
  {   // the counter fails in round 1: nothing has changed
    Scene S, same;
    sceneC(S);
    sceneC(same);
    orbfe::KeyFrameCullingStats st = {-1, -1, -1};
    gCalls = 0, gFailAt = 1;
    CHECK(orbfe::KeyFrameCullingWith(failing, S.local, &st) == ORBFE_ERR_HIP && st.calls == 0 && st.culled == 0 && S.state() == same.state());
    // in round 2: A's cull stands, as it would after the first step of the sequential loop; nothing else has changed
    gCalls = 0, gFailAt = 2;
    CHECK(orbfe::KeyFrameCullingWith(failing, S.local, &st) == ORBFE_ERR_HIP && st.calls == 1 && st.culled == 1);
    same.local[0]->SetBadFlag();
    CHECK(S.state() == same.state());
  }
  std::printf("PASS\n");
  return 0;
}
