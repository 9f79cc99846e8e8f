"""CPU side of the covisibility counts (orbfe_covisibility_counts): the restatement tests/cpp/covisibility_ref.cpp against an
independent numpy count; the host-side bookkeeping os1_amd/csrc/covis_plan.h and the facade include/orbfe/Covisibility.h as
stand-alone programs with the address and undefined-behaviour sanitizers linked in (nothing loaded into Python runs under a
sanitizer); the C ABI's argument check through the library, which refuses before it looks at the matcher; the header as C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covisibility_util as U


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('covis_ref'))


@pytest.fixture(scope='module')
def api():
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    api.load_library()
    return api


def same(a, b):
    return all(x.dtype == y.dtype and x.tolist() == y.tolist() for x, y in zip(a, b))


def test_restatement_equals_the_numpy_count(ref):
    special, names = U.special_case()
    cases = [special, U.small_map(), U.random_case(1, 1, 1), U.random_case(2, 65, 130), U.random_case(3, 300, 7, must=(0, 299))]
    for c in cases:
        assert same(U.ref_counts(ref, c), U.np_counts(c))
    k = np.arange(65, dtype=np.int32)
    base = U.random_case(4, 65, 65, frames=0.0)
    for limits in (np.zeros(65, np.int32), k + 1, np.full(65, 65, np.int32), None):
        c = base.with_limits(limits)
        assert same(U.ref_counts(ref, c), U.np_counts(c))
    assert U.ref_counts(ref, base.with_limits(np.zeros(65, np.int32)))[0].tolist() == [0] * 66


def test_special_subjects_in_the_restatement(ref):
    c, names = U.special_case()
    offs, kf, cnt = U.ref_counts(ref, c)
    seg = {n: (kf[offs[s]:offs[s + 1]].tolist(), cnt[offs[s]:offs[s + 1]].tolist()) for s, n in enumerate(names)}
    for n in ('no_entries', 'all_skipped', 'zero_observations', 'only_itself'):
        assert seg[n] == ([], []), n
    assert seg['named_300_times'] == ([0, 1, 2, 4, 64, 65, 69], [1, 300, 300, 300, 300, 300, 1])
    assert seg['frame'][0][:6] == [0, 1, 2, 3, 4, 5] and seg['frame'][1][3] == 4      # slot 3: MapPoints 0, 3, 3 and 4
    assert 69 not in seg['plain'][0]
    # the overflow report of the restatement: the count is right whatever the room
    total = int(offs[-1])
    assert U.ref_counts(ref, c, cap=total) == (0, total) and U.ref_counts(ref, c, cap=total - 1) == (-5, total)


def test_bound_is_never_exceeded(ref, api):
    special, _ = U.special_case()
    for c in (special, U.small_map(), U.random_case(2, 65, 130), U.random_case(4, 65, 65).with_limits(np.arange(65) + 1)):
        offs, _, _ = U.ref_counts(ref, c)
        assert int(offs[-1]) <= api.covisibility_bound(c.n_kf, c.obs_offsets, c.subj_offsets, c.subj_mp, c.subj_limit)


def test_plan_header_under_the_sanitizers(tmp_path):
    U.run(U.compile_plan_test(str(tmp_path / 'covis_plan')))


def test_facade_header_compiles_and_runs_on_the_restated_back_end(tmp_path):
    U.syntax_check()
    U.run(U.compile_facade(str(tmp_path / 'covis_host'), host_backend=True, sanitize=True))


def test_arguments_are_refused_before_the_matcher_is_looked_at(api):
    c, _ = U.special_case()

    def refused(word, matcher=None, cap=None, **change):
        d = U.Case.__new__(U.Case)
        d.__dict__.update(c.__dict__)
        for k, (i, v) in change.items():
            a = getattr(d, k).copy()
            a[i] = v
            setattr(d, k, a)
        with pytest.raises(api.OrbfeError) as e:
            api.covisibility_counts(matcher, *d.args(), cap=cap)
        assert e.value.code == -1 and word in str(e.value), e.value

    refused('null pointer (matcher)')                                    # valid arrays: the matcher is the only objection
    refused('obs_offsets decreases', obs_offsets=(2, 1))
    refused('subj_offsets decreases', subj_offsets=(3, 10))
    refused('obs_kf[2] = 70', obs_kf=(2, 70))
    refused('obs_kf[0] = -1', obs_kf=(0, -1))
    refused('subj_mp[40] = 6', subj_mp=(40, 6))
    refused('subj_mp[40] = -2', subj_mp=(40, -2))
    refused('subj_self[1] = 70', subj_self=(1, 70))
    refused('subj_self[1] = -2', subj_self=(1, -2))
    refused('negative size', cap=-1)
    L = api.load_library()
    d = c.with_limits(np.full(c.n_subj, c.n_kf, np.int32))
    for i, v, word in ((0, 71, 'subj_limit[0] = 71'), (2, -1, 'subj_limit[2] = -1')):
        lim = d.subj_limit.copy()
        lim[i] = v
        with pytest.raises(api.OrbfeError) as e:
            api.covisibility_counts(None, *d.with_limits(lim).args())
        assert e.value.code == -1 and word in str(e.value)
    # sizes and pointers, straight through the C ABI
    out = np.zeros(8, np.int32)
    need = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data
    good = [None, c.n_kf, c.n_mp, p(c.obs_offsets), p(c.obs_kf), c.n_subj, p(c.subj_self), None, p(c.subj_offsets), p(c.subj_mp), p(out), p(out),
            p(out), 0, need.ctypes.data_as(C.POINTER(C.c_int))]
    for at, v, word in ((1, -1, 'negative size'), (2, -1, 'negative size'), (5, -1, 'negative size'), (3, None, 'null pointer'),
                        (4, None, 'null pointer'), (6, None, 'null pointer'), (8, None, 'null pointer'), (9, None, 'null pointer'),
                        (10, None, 'null pointer'), (14, None, 'null pointer')):
        a = list(good)
        a[at] = v
        assert L.orbfe_covisibility_counts(*a) == -1 and word in L.orbfe_last_error().decode(), (at, L.orbfe_last_error())
    a = list(good)
    a[13], a[11] = 5, None                                                # room for entries but nowhere to put them
    assert L.orbfe_covisibility_counts(*a) == -1 and 'null pointer' in L.orbfe_last_error().decode()
    a = list(good)
    a[5] = 0                                                              # n_subj == 0 is fine -- for a matcher
    assert L.orbfe_covisibility_counts(*a) == -1 and 'matcher' in L.orbfe_last_error().decode()


def test_slots_per_pass_leaves_room_for_two_workgroups_per_cu(api):
    slots = api.covis_slots_per_pass()
    lds_per_cu = 160 * 1024
    assert slots >= 1024 and 2 * (4 * slots + 64) <= lds_per_cu


def test_header_still_compiles_as_c(tmp_path):
    p = str(tmp_path / 't.c')
    open(p, 'w').write('#include "orbfe.h"\nint main(void) { return (int)sizeof(&orbfe_covisibility_counts) - (int)sizeof(&orbfe_debug_covis_slots_per_pass)'
                       ' + (int)sizeof(&orbfe_debug_covis_ms) - 8; }\n')
    subprocess.check_call(['gcc', '-x', 'c', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(U.ROOT, 'include'), p])
