"""CPU side of the MapPoint refresh (orbfe_local_map_refresh_rows): the restatement tests/cpp/map_point_refresh_ref.cpp against
the oracle's ComputeDistinctiveDescriptors and against a numpy float32 / float64 emulation of the UpdateNormalAndDepth chain;
the facade header include/orbfe/MapPointRefresh.h on the new stub, syntax and a run on the restated back end; the C ABI's
argument check; the header as C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_point_refresh_util as U

f32 = np.float32


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('mpr_ref'))


@pytest.fixture(scope='module')
def scene():
    return U.make_scene()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_best_index_equals_the_oracle_on_the_filtered_list(ref, scene, oracle):
    kfs, table, b = scene
    _, best, _, _, _, rc = U.ref_refresh(ref, table, U.DESCRIPTOR, kfs, b)
    assert rc == 0
    some = 0
    for p, o in enumerate(b.obs_lists):
        kept = [i for i, t in enumerate(o) if not t[2]]
        if not kept:
            assert best[p] == -1, b.names[p]
            continue
        descs = np.stack([kfs[o[i][0]].desc[o[i][1]] for i in kept])
        want = oracle.distinctive_descriptor(descs)
        assert best[p] == kept[want], b.names[p]
        some += 1
    assert some >= len(U.N_SHAPES) + 5
    # ties go to the first: the two copies of 'all_equal' have median 0 both
    assert best[b.names.index('all_equal')] == 0


def test_descriptor_rows_hold_the_winner_and_all_bad_lists_keep_theirs(ref, scene):
    kfs, table, b = scene
    t, best, nrm, mn, mx, rc = U.ref_refresh(ref, table, U.DESCRIPTOR | U.NORMAL_DEPTH, kfs, b)
    assert rc == 0
    for p, o in enumerate(b.obs_lists):
        r = b.rows[p]
        assert t[r, :12].tobytes() == table[r, :12].tobytes()                      # pos is never written
        if best[p] >= 0:
            s, k, _ = o[best[p]]
            assert t[r, 32:].tobytes() == kfs[s].desc[k].tobytes(), b.names[p]
        else:
            assert t[r, 32:].tobytes() == table[r, 32:].tobytes(), b.names[p]
        if o:
            assert t[r, 12:32].tobytes() != table[r, 12:32].tobytes(), b.names[p]   # normal and depth change, bad lists included
        else:
            assert t[r].tobytes() == table[r].tobytes()
    p = b.names.index('all_bad')
    assert best[p] == -1 and t[b.rows[p], 32:].tobytes() == table[b.rows[p], 32:].tobytes()
    untouched = np.setdiff1d(np.arange(U.CAPACITY), b.rows)
    assert t[untouched].tobytes() == table[untouched].tobytes()


def test_normal_and_depth_equal_the_numpy_chain(ref, scene):
    kfs, table, b = scene
    t, _, nrm, mn, mx, rc = U.ref_refresh(ref, table, U.NORMAL_DEPTH, kfs, b)
    assert rc == 0
    tf = table.view(f32).reshape(-1, 16)
    for p, o in enumerate(b.obs_lists):
        if not o:
            continue
        pos = tf[b.rows[p], 0:3]
        Ow = np.stack([kfs[s].Ow for s, _, _ in o])
        level = kfs[b.ref_kf[p]].oct[b.ref_kp[p]]
        wn, wmn, wmx = U.np_normal_depth(pos, Ow, kfs[b.ref_kf[p]].Ow, U.SF[level], U.SF[-1])
        assert bits(nrm[p]).tolist() == bits(wn).tolist(), b.names[p]
        assert bits(mn[p]) == bits(wmn) and bits(mx[p]) == bits(wmx), b.names[p]
        row = t.view(f32).reshape(-1, 16)[b.rows[p]]
        assert bits(row[3:6]).tolist() == bits(wn).tolist() and bits(row[6]) == bits(wmn) and bits(row[7]) == bits(wmx)
        assert t[b.rows[p], 32:].tobytes() == table[b.rows[p], 32:].tobytes()      # DESCRIPTOR not selected


def test_reciprocal_of_the_norm_is_not_representable(ref):
    # |(1, 1, 1)| = sqrt(3): 1.0/sqrt(3) is rounded to float before the products; and |(3, 4, 0)| = 5, whose reciprocal no
    # binary float holds either
    for pos, Ow in (((1, 2, 3), (0, 1, 2)), ((3, 4, 0), (0, 0, 0))):
        n, mn, mx = U.ref_normal_depth(ref, pos, [Ow], Ow, 1.2, U.SF[-1])
        wn, wmn, wmx = U.np_normal_depth(pos, [Ow], Ow, 1.2, U.SF[-1])
        assert bits(n).tolist() == bits(wn).tolist() and bits(mn) == bits(wmn) and bits(mx) == bits(wmx)
    beta = f32(1.0 / np.sqrt(3.0))
    n, _, _ = U.ref_normal_depth(ref, (1, 2, 3), [(0, 1, 2)], (0, 1, 2), 1.0, 1.0)
    assert bits(n).tolist() == bits(np.full(3, beta, f32)).tolist()
    assert float(beta) != 1.0 / np.sqrt(3.0)
    # a float division by the norm would give another last bit somewhere on this sweep; the stated chain multiplies by beta
    rng = np.random.default_rng(3)
    differs = 0
    for _ in range(200):
        pos, Ow = rng.uniform(-5, 5, 3).astype(f32), rng.uniform(-1, 1, 3).astype(f32)
        n, _, _ = U.ref_normal_depth(ref, pos, [Ow], Ow, 1.0, 1.0)
        wn, _, _ = U.np_normal_depth(pos, [Ow], Ow, 1.0, 1.0)
        assert bits(n).tolist() == bits(wn).tolist()
        ni = pos - Ow
        differs += bits(ni / f32(np.sqrt(np.sum(ni.astype(np.float64) ** 2)))).tolist() != bits(wn).tolist()
    assert differs > 0


def test_minus_zero_becomes_plus_zero(ref):
    # the x component sums to the smallest negative denormal; halved it rounds to -0, and convertTo's `+ 0` makes it +0
    pos, Ow = (0, 0, 2), [(f32(2.8e-45), 0, 0), (0, 0, 0)]
    n, _, _ = U.ref_normal_depth(ref, pos, Ow, Ow[1], 1.0, 1.0)
    wn, _, _ = U.np_normal_depth(pos, Ow, Ow[1], 1.0, 1.0)
    assert bits(n).tolist() == bits(wn).tolist()
    assert bits(n)[0] == 0 and bits(n)[1] == 0 and n[2] == 1.0
    with np.errstate(under='ignore'):
        assert bits(f32(-1.4e-45) * f32(0.5)) == 0x80000000                        # (what the product alone gives)


def test_out_of_range_level_leaves_the_row(ref, scene):
    kfs, table, b = scene
    t, _, _, _, _, rc = U.ref_refresh(ref, table, U.DESCRIPTOR | U.NORMAL_DEPTH, kfs, b, nlevels=4, sf=U.SF[:4])
    levels = [kfs[b.ref_kf[p]].oct[b.ref_kp[p]] if o else 0 for p, o in enumerate(b.obs_lists)]
    bad = [p for p, l in enumerate(levels) if l >= 4]
    assert bad and rc == -1 - bad[0]
    for p in bad:
        assert t[b.rows[p]].tobytes() == table[b.rows[p]].tobytes()


def test_facade_header_compiles_and_runs_on_the_restated_back_end(tmp_path):
    U.syntax_check()
    U.run_facade(U.compile_facade(str(tmp_path / 'mpr_host'), host_backend=True))


def test_null_matcher_is_refused():
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    L = C.CDLL(api.lib_path())
    L.orbfe_local_map_refresh_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_int] + [C.c_void_p] * 11
    L.orbfe_last_error.restype = C.c_char_p
    rows = np.zeros(1, np.int32)
    offs = np.zeros(2, np.int32)
    rc = L.orbfe_local_map_refresh_rows(None, None, 3, 0, None, None, None, 8, 1, rows.ctypes.data, offs.ctypes.data, *([None] * 9))
    assert rc == -1 and L.orbfe_last_error()
    L.orbfe_local_map_download_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.orbfe_local_map_download_rows(None, 1, rows.ctypes.data, rows.ctypes.data) == -1


def test_header_still_compiles_as_c(tmp_path):
    p = str(tmp_path / 't.c')
    open(p, 'w').write('#include "orbfe.h"\nint main(void) { return ORBFE_REFRESH_DESCRIPTOR + ORBFE_REFRESH_NORMAL_DEPTH + (int)ORBFE_OBS_KF_BAD - 4 +'
                       ' (int)sizeof(&orbfe_local_map_refresh_rows) - (int)sizeof(&orbfe_local_map_download_rows); }\n')
    subprocess.check_call(['gcc', '-x', 'c', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(U.ROOT, 'include'), p])
