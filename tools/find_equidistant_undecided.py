#!/usr/bin/env python3
"""Find inputs the equidistant kernel cannot decide (os1_amd/csrc/equidistant_tan.h) and write tests/golden/equidistant_undecided.npz.

  free points    uniform float32 points around the 640 x 480 image under the Sony AS-20 camera: every undecided one is confirmed with
                 mpmath at 60 digits and sorted by axis and by whether the correctly rounded tan gives the UPPER float (the kernel's
                 provisional value, the lowest candidate's, is then wrong and the host settle must change it) or the lower.
  camera centres principal points (cx, cy) that make one chosen pixel undecided-upper: the pixel is a level-0 keypoint of BOTH frame 1
                 and frame 2 of tests/undistort_stream_util.py's scene, so one camera gives the settle test a patched point in the
                 middle of a batch and one in a batch's last frame.

Prints the measured undecided rate of the free scan.  --coefficients prints the double-double Taylor coefficients of the header."""
import argparse
import os
import subprocess
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import equidistant_util as E  # noqa: E402


def coefficients():
    mp.mp.prec = 400
    for name, first in (('kS', 1), ('kC', 0)):
        print(name)
        for k in range(15 if first else 16):
            v = mp.mpf((-1) ** k) / mp.factorial(2 * k + first)
            h = float(v)
            print('  {%s, %s},' % (float.hex(h), float.hex(float(v - mp.mpf(h)))))


def scan(mode, a, b, box, seed, count, threads):
    out = subprocess.check_output([E.program(fast=True), mode, repr(E.SONY[0]), repr(E.SONY[1]), repr(a), repr(b)] +
                                  [repr(float(v)) for v in box] + [str(seed), str(count), str(threads)], text=True).split('\n')
    pts = [tuple(float.fromhex(w) for w in line.split()) for line in out if line.startswith(('0x', '-0x'))]
    return np.asarray(pts, np.float32).reshape(-1, 2)


def shared_keypoint():
    """A level-0 pixel that is a keypoint of frame 1 and of frame 2."""
    import undistort_stream_util as U
    from oracle.pyoracle import Oracle
    ex = U.extracted(Oracle())
    sets = [{(float(k['x']), float(k['y'])) for k in kps[kps['octave'] == 0]} for kps, _ in ex]
    both = sorted(sets[1] & sets[2])
    if not both:
        raise SystemExit('frames 1 and 2 share no level-0 keypoint position')
    return both[len(both) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--coefficients', action='store_true')
    ap.add_argument('--count', type=int, default=400_000_000)
    ap.add_argument('--threads', type=int, default=8)
    ap.add_argument('--per-class', type=int, default=8)
    a = ap.parse_args()
    if a.coefficients:
        return coefficients()
    need = a.per_class
    groups = {(ax, kind): [] for ax in 'xy' for kind in ('upper', 'lower')}
    scanned = found = 0
    seed = 1
    while min(len(v) for v in groups.values()) < need:
        pts = scan('scan', E.SONY[2], E.SONY[3], (-40, 680, -40, 520), seed, a.count, a.threads)
        scanned += a.count
        seed += 1
        for u, v in pts:
            und, kinds, _ = E.classify(E.SONY, u, v)
            if not und:       # undecided for the header only because its enclosure straddles a double: not golden material
                continue
            found += 1
            for ax, kind in zip('xy', kinds):
                if kind and len(groups[(ax, kind)]) < 2 * need:
                    groups[(ax, kind)].append((u, v))
    print('free scan: %d points, %d confirmed undecided: rate %.3g per point' % (scanned, found, found / scanned))
    u, v = shared_keypoint()
    centres = []
    seed = 100
    while len(centres) < 2:
        for cx, cy in scan('centres', u, v, (E.SONY[2] - 8, E.SONY[2] + 8, E.SONY[3] - 8, E.SONY[3] + 8), seed, a.count // 4, a.threads):
            cam = (E.SONY[0], E.SONY[1], cx, cy)
            und, kinds, _ = E.classify(cam, u, v)
            if und and 'upper' in kinds:
                centres.append((cx, cy))
        seed += 1
    print('pixel (%g, %g): %d centres make it undecided-upper' % (u, v, len(centres)))
    np.savez(E.GOLDEN, camera=np.asarray(E.SONY, np.float32), pixel=np.asarray((u, v), np.float32),
             centres=np.asarray(centres, np.float32),
             **{'%s_%s' % k: np.asarray(p, np.float32) for k, p in groups.items()})
    print('wrote', E.GOLDEN)


if __name__ == '__main__':
    main()
