"""tests/manager_terms_reference.py against the reference's own mdp/rewards.py, as recorded by
tools/gen_manager_terms_goldens.py in tests/golden/mdp_manager_terms.npz (32 envs x 16 random calls, then
three calls of constructed rows): continuous terms to 1e-6 absolute, the gait count and every gate
bit-exact."""
import json
import os

import numpy as np
import pytest

import manager_terms_reference as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "mdp_manager_terms.npz")
EDGE_EP_LEN = [0, 27, 28, 49, 50, 55, 77, 78, 99, 100, 155]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def evaluated(gold):
    """The float64 reference on every call's inputs, the integrator carried as the goldens carried it."""
    g = gold
    out, after = [], []
    for t in range(len(g["in_ep_len"])):
        fwd = ref.forward_xy(g["in_root_quat"][t])
        v, s = ref.terms(g["in_ep_len"][t], float(g["step_dt"]), g["in_cmd"][t], g["in_contact_time"][t],
                         g["in_air_time"][t], g["in_foot_z"][t], g["in_foot_vxy"][t], fwd, g["in_root_vel"][t],
                         g["in_fz_hist"][t], g["force_sum_before"][t])
        out.append(v)
        after.append(s)
    return np.stack(out), np.stack(after)


def test_goldens_hold_the_base_cfg(gold):
    rec = json.loads(str(gold["config_json"]))
    p = ref.Params()
    assert list(gold["term_names"]) == ref.TERMS
    assert rec["gait"]["func"] == "feet_gait" and rec["gait"]["weight"] == 0.5
    assert rec["gait"]["params"] == {"period": p.gait_period, "offset": list(p.gait_offset),
                                     "threshold": p.gait_threshold, "command_name": "base_velocity"}
    assert rec["feet_clearance"]["func"] == "foot_clearance_reward"
    assert rec["feet_clearance"]["params"] == {"std": p.clearance_std, "tanh_mult": p.clearance_tanh_mult,
                                               "target_height": p.clearance_target_height}
    assert rec["feet_air_time"]["func"] == "feet_air_time_positive_biped" and rec["feet_air_time"]["weight"] == 2.5
    assert rec["feet_air_time"]["params"] == {"command_name": "base_velocity", "threshold": p.air_time_threshold}
    assert rec["base_vel_forward"] == {"func": "base_vel_forward", "weight": 1.0, "params": {"which_forward": 1}}
    assert rec["feet_force_pattern"]["func"] == "feet_force_pattern" and rec["feet_force_pattern"]["weight"] == 1.0
    from zbot_lab_amd import model as zm
    order = [k for k in gold["reward_field_order"] if k != "undesired_contacts"]
    assert order == zm.M_REWARD_FIELD_ORDER and zm.M_EXTRA_REWARD_TERMS == ref.TERMS


def test_continuous_terms_to_1e_6(gold, evaluated):
    v, after = evaluated
    for k in (1, 2, 3, 4):
        err = np.abs(v[..., k] - gold["terms"][..., k]).max()
        print(ref.TERMS[k], "max abs error", err)
        assert err <= 1e-6, ref.TERMS[k]
    assert np.abs(after - gold["force_sum_after"]).max() <= 1e-6


def test_gait_count_is_bit_exact(gold, evaluated):
    v, _ = evaluated
    assert np.array_equal(v[..., 0].astype(np.float32), gold["terms"][..., 0])
    assert set(np.unique(gold["terms"][..., 0])) == {0.0, 1.0, 2.0}


def test_gait_phase_edges_follow_the_fp32_arithmetic(gold):
    """The constructed call holds every edge value of episode_length_buf; of them only 155 is decided by
    the rounding of ep * 0.02 in fp32 (at 55 the fp32 phase and exact arithmetic decide alike)."""
    t = int(gold["num_random_calls"])
    ep = gold["in_ep_len"][t]
    assert set(ep) == set(EDGE_EP_LEN)
    g = ref.gates(ep, float(gold["step_dt"]), gold["in_cmd"][t], gold["in_contact_time"][t], ref.Params())
    assert g["moving3"].all()
    count = (g["stance"] == g["in_contact"]).sum(-1)
    assert np.array_equal(count.astype(np.float32), gold["terms"][t, :, 0])
    pats = {tuple(r) for r in g["in_contact"]}
    assert pats == {(True, True), (True, False), (False, True), (False, False)}
    # the exact-arithmetic decision differs from the recorded one somewhere among the edges, or agrees
    # everywhere: either way the fp32 restatement is the one that matches (asserted above); show which
    exact = np.stack([((ep * 0.02 % 2.0) / 2.0 + o) % 1.0 < 0.55 for o in (0.0, 0.5)], -1)
    differ = sorted(set(int(x) for x in ep[(exact != g["stance"]).any(-1)]))
    print("edge rows where exact arithmetic and fp32 disagree:", differ)
    assert differ == [155]


def test_command_and_timer_gates_are_bit_exact(gold):
    t = int(gold["num_random_calls"]) + 1
    p = ref.Params()
    g = ref.gates(gold["in_ep_len"][t], float(gold["step_dt"]), gold["in_cmd"][t], gold["in_contact_time"][t], p)
    # both sides of both thresholds, and the thresholds themselves, are present
    assert {0.0499, 0.05, 0.0501, 0.0999, 0.1, 0.1001} <= {round(float(x), 4) for x in g["norm3"]}
    assert g["moving3"].any() and not g["moving3"].all() and g["moving2"].any() and not g["moving2"].all()
    gait_on = gold["terms"][t, :, 0] != 0
    count = (g["stance"] == g["in_contact"]).sum(-1)
    assert np.array_equal(gait_on, g["moving3"] & (count > 0))
    air_on = gold["terms"][t, :, 2] != 0
    assert np.array_equal(air_on, g["moving2"] & g["single_stance"])
    times = np.concatenate([gold["in_contact_time"][t], gold["in_air_time"][t]], -1)
    assert (times > p.air_time_threshold).any() and ((times > 0) & (times < p.air_time_threshold)).any()
    assert gold["terms"][t, :, 2].max() == np.float32(p.air_time_threshold)


def test_force_pattern_sign_cases_and_reset(gold, evaluated):
    t = int(gold["num_random_calls"]) + 2
    before = gold["force_sum_before"][t]
    assert (before == 0).any() and (before > 0).any() and (before < 0).any()
    # sign(0) = 0: the difference term vanishes, the penalty reads the integrator after its update
    z = before == 0
    F = gold["in_fz_hist"][t].astype(np.float64).mean(1)
    assert np.allclose(gold["terms"][t, z, 4], -0.1 * np.abs(0.001 * (F[z, 0] - F[z, 1])), atol=1e-6)
    # reset_my_data zeroed the integrator of the reset envs between two calls (random and constructed)
    for call in np.nonzero(gold["resets"].any(1))[0]:
        ids = gold["resets"][call]
        assert (gold["force_sum_before"][call][ids] == 0).all()
        if call != t:
            assert (gold["force_sum_after"][call - 1][ids] != 0).all()
    keep = ~gold["resets"][1:]
    assert np.array_equal(gold["force_sum_before"][1:t][keep[:t - 1]], gold["force_sum_after"][:t - 1][keep[:t - 1]])


def test_float32_statement_tracks_float64(gold, evaluated):
    """The same statement in float32 (what sizes the GPU tolerance) stays within a few ulp of float64."""
    v64, _ = evaluated
    t = 3
    fwd = ref.forward_xy(gold["in_root_quat"][t], np.float32)
    v32, _ = ref.terms(gold["in_ep_len"][t], float(gold["step_dt"]), gold["in_cmd"][t], gold["in_contact_time"][t],
                       gold["in_air_time"][t], gold["in_foot_z"][t], gold["in_foot_vxy"][t], fwd, gold["in_root_vel"][t],
                       gold["in_fz_hist"][t], gold["force_sum_before"][t], dtype=np.float32)
    assert v32.dtype == np.float32
    assert np.abs(v32 - v64[t]).max() < 5e-6


def test_sensor_update_law():
    """ContactSensor: exactly one of the two current timers of a foot is positive after an update; the
    last air time latches at touch-down."""
    rng = np.random.default_rng(0)
    a = l = c = np.zeros((64, 2), np.float32)
    for _ in range(50):
        hit = rng.random((64, 2)) < 0.5
        a0 = a
        a, l, c = ref.sensor_update(a, l, c, hit, 0.005)
        assert ((a > 0) ^ (c > 0)).all() and ((c > 0) == hit).all()
        latch = (a0 > 0) & hit
        assert np.array_equal(l[latch], (a0 + np.float32(0.005))[latch])
