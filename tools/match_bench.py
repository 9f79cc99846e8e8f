"""Developer timing helper (GPU box): batched SearchForInitialization cost (the host-array search) and the cost of one projected
search on a resident frame."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from os1_amd import api
from os1_amd.synth import synth, shifted
B = 16
W, H, N = 1920, 1080, 2000
base = synth(100, W, H)
frames = [base] + [shifted(base, 2 * i, i, 100000 + i) for i in range(1, B)]
ex = api.Extractor(N, 1.2, 8, 20, 7)
feats = ex.extract_batch(frames)
mt = api.Matcher()
bounds = (0.0, float(W), 0.0, float(H))
pairs = []
for i in range(B):
    k1, d1 = feats[i - 1]; k2, d2 = feats[i]
    pairs.append((k1, d1, k2, d2, np.stack([k1['x'], k1['y']], 1)))
for _ in range(3): r = mt.search_for_initialization_batch(pairs, bounds)
R = 20
ts = []
for _ in range(R):
    t = time.perf_counter()
    r = mt.search_for_initialization_batch(pairs, bounds)
    ts.append(time.perf_counter() - t)
dt = float(np.median(ts))
print('stages ms (arena, gpu, resolve):', mt.stage_ms())
print('batch of %d pairs: median %.3f ms  (%.1f us/pair, min %.3f ms)  matches %s' % (B, dt * 1e3, dt / B * 1e6, min(ts) * 1e3, [x[0] for x in r][:6]))
t = time.time()
for _ in range(R):
    for p in pairs[:4]: mt.search_for_initialization(p[0], p[1], p[2], p[3], bounds, p[4])
print('single pair: %.1f us' % ((time.time() - t) / R / 4 * 1e6))
# resident frame: frame 1 on the device, every keypoint of frame 0 a query at its own position, radius 15 * 1.2^octave
(k1, d1), (k2, d2) = feats[0], feats[1]
fr = api.Frame.from_host(mt, k2, d2, bounds)
uv = np.stack([k1['x'], k1['y']], 1).astype(np.float32)
radius = (15.0 * 1.2 ** k1['octave']).astype(np.float32)
level, valid = k1['octave'].astype(np.int32), np.ones(len(k1), np.uint8)
for _ in range(20): g = mt.search_projected(fr, None, None, uv, radius, level, valid, d1, None, True, None, 5.99, 50)
ts = []
for _ in range(200):
    t = time.perf_counter()
    g = mt.search_projected(fr, None, None, uv, radius, level, valid, d1, None, True, None, 5.99, 50)
    ts.append(time.perf_counter() - t)
print('resident frame, %d queries: median %.1f us  (min %.1f)  matches %d' % (len(k1), np.median(ts) * 1e6, min(ts) * 1e6, g[0]))
