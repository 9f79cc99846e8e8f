"""CPU side of the keyframe-culling counts (orbfe_redundant_observations) and of include/orbfe/KeyFrameCulling.h: the restatement
tests/cpp/keyframe_culling_ref.cpp against hand-worked figures and an independent numpy count; the host-side argument check
os1_amd/csrc/culling_plan.h and the facade as stand-alone programs, built plainly and with the address and undefined-behaviour
sanitizers linked in (nothing loaded into Python runs under a sanitizer); the facade's sequential logic on stub maps with the
restated counter against the sequential loop; the C ABI's argument check through the library, which refuses before it looks at
the matcher; the call site of INTEGRATION.md against the stubs; the header as C."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_culling_util as U


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('kfcull_ref'))


@pytest.fixture(scope='module')
def api():
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    api.load_library()
    return api


def pairs(counts):
    return list(zip(counts[0].tolist(), counts[1].tolist()))


@pytest.mark.parametrize('th_obs', (1, 3))
def test_restatement_gives_the_hand_worked_figures(ref, th_obs):
    c, names, want = U.crafted_case(th_obs)
    got = pairs(U.ref_counts(ref, c))
    assert dict(zip(names, got)) == dict(zip(names, want))
    assert pairs(U.ref_counts(ref, c, structs=True)) == want and pairs(U.np_counts(c)) == want
    assert pairs(U.ref_counts(ref, c.rebased())) == want
    lengths = set(np.diff(c.obs_offsets).tolist())
    assert {0, th_obs, th_obs + 1, U.LONG, U.LONG + 1, 300} <= lengths               # both sides of the long-list route


def test_restatement_with_observation_counts_of_their_own(ref):
    c, want = U.nobs_case()
    assert pairs(U.ref_counts(ref, c)) == want and pairs(U.ref_counts(ref, c, structs=True)) == want and pairs(U.np_counts(c)) == want
    assert pairs(U.ref_counts(ref, c.but(mp_nobs=None))) == [(4, 2)]                    # MapPoints 1 and 3 then, not 0 and 3
    assert pairs(U.ref_counts(ref, c.but(mp_nobs=np.array([4, 4, 9, 4], np.int32)))) == [(4, 3)]


def test_restatement_equals_the_numpy_count_on_a_random_map(ref):
    for th in (1, 3):
        c = U.random_map(th_obs=th)
        assert c.n_kf == 40 and (np.diff(c.subj_offsets) == 300).all()
        a = U.ref_counts(ref, c)
        assert pairs(a) == pairs(U.np_counts(c)) == pairs(U.ref_counts(ref, c, structs=True))
        assert 0 < a[1].sum() < a[0].sum()


def test_plan_header_plain_and_under_the_sanitizers(tmp_path):
    U.run(U.compile_plan_test(str(tmp_path / 'culling_plan'), sanitize=False))
    U.run(U.compile_plan_test(str(tmp_path / 'culling_plan_san'), sanitize=True))


def test_facade_on_stub_maps_equals_the_sequential_loop(tmp_path):
    U.run(U.compile_facade(str(tmp_path / 'kfcull_host'), gpu=False))
    U.run(U.compile_facade(str(tmp_path / 'kfcull_host_san'), gpu=False, sanitize=True))


def test_integration_call_site_type_checks_against_the_stubs():
    U.syntax_check_call_site()
    text = open(os.path.join(U.ROOT, 'INTEGRATION.md')).read()
    src = open(os.path.join(U.CPP, 'keyframe_culling_callsite.cpp')).read()
    line = 'orbfe::KeyFrameCulling(matcher, vpLocalKeyFrames);'
    assert line in text and line in src


def test_arguments_are_refused_before_the_matcher_is_looked_at(api):
    c, _, _ = U.crafted_case()

    def refused(word, **change):
        d = c.but()
        for k, v in change.items():
            if isinstance(v, tuple):
                a = getattr(d, k).copy()
                a[v[0]] = v[1]
                v = a
            setattr(d, k, v)
        with pytest.raises(api.OrbfeError) as e:
            api.redundant_observations(None, *d.args())
        assert e.value.code == -1 and word in str(e.value), e.value

    refused('null pointer (matcher)')                                    # valid arrays: the matcher is the only objection
    refused('obs_offsets decreases', obs_offsets=(3, 1))
    refused('subj_offsets decreases', subj_offsets=(3, 100))
    refused('obs_kf[2] = 400', obs_kf=(2, 400))
    refused('obs_kf[0] = -1', obs_kf=(0, -1))
    refused('subj_mp[40] = %d' % c.n_mp, subj_mp=(40, c.n_mp))
    refused('subj_mp[40] = -2', subj_mp=(40, -2))
    refused('subj_self[1] = 400', subj_self=(1, 400))
    refused('subj_self[1] = -2', subj_self=(1, -2))
    refused('th_obs = 0', th_obs=0)
    nobs = np.diff(c.obs_offsets).astype(np.int32)
    nobs[5] = -1
    refused('mp_nobs[5] = -1', mp_nobs=nobs)
    # sizes and pointers, straight through the C ABI
    L = api.load_library()
    out = np.zeros(c.n_subj, np.int32)
    p = lambda a: a.ctypes.data
    good = [None, c.n_kf, c.n_mp, p(c.obs_offsets), p(c.obs_kf), p(c.obs_level), None, c.n_subj, p(c.subj_self), p(c.subj_offsets), p(c.subj_mp),
            p(c.subj_level), 3, p(out), p(out)]
    for at, v, word in ((1, -1, 'negative size'), (2, -1, 'negative size'), (7, -1, 'negative size'), (3, None, 'null pointer'),
                        (4, None, 'null pointer'), (5, None, 'null pointer'), (8, None, 'null pointer'), (9, None, 'null pointer'),
                        (10, None, 'null pointer'), (11, None, 'null pointer'), (13, None, 'null pointer'), (14, None, 'null pointer'),
                        (12, 0, 'th_obs')):
        a = list(good)
        a[at] = v
        assert L.orbfe_redundant_observations(*a) == -1 and word in L.orbfe_last_error().decode(), (at, L.orbfe_last_error())
    a = list(good)
    a[7] = 0                                                              # n_subj == 0 is fine -- for a matcher
    assert L.orbfe_redundant_observations(*a) == -1 and 'matcher' in L.orbfe_last_error().decode()


def test_header_still_compiles_as_c(tmp_path):
    p = str(tmp_path / 't.c')
    open(p, 'w').write('#include "orbfe.h"\nint main(void) { return (int)sizeof(&orbfe_redundant_observations) - (int)sizeof(&orbfe_debug_culling_ms); }\n')
    subprocess.check_call(['gcc', '-x', 'c', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(U.ROOT, 'include'), p])
