"""The host statement of the footprint collision test (rift_amd/planning/fine_tuner/rlft/traj_eval/footprint.py; include/rift_footprint.h
states the rule) against exact arithmetic, and the cases of tests/footprint_cases.py against what they claim.  No GPU."""
import numpy as np
import pytest
import torch

from tests import footprint_cases as F


def _fp():
    from rift_amd.planning.fine_tuner.rlft.traj_eval import footprint
    return footprint


def test_known_pairs_are_what_they_claim():
    """Dyadic coordinates (multiples of 2^-4, |x| <= 64, exact in fp32); the exact segment-crossing / containment test gives the stated
    answer; every base pair comes as given, rewound and exchanged; the set holds colliding, touching and clear pairs, and clear pairs whose
    envelopes meet."""
    pairs = F.known_pairs()
    assert len(pairs) == 3 * len(F._BASE) >= 30
    for name, P, Q, hit, env in pairs:
        for quad in (P, Q):
            q = np.asarray(quad, dtype=np.float64)
            assert q.shape == (4, 2) and np.array_equal(q * 16, np.rint(q * 16)) and np.abs(q).max() <= 64, name
            assert np.array_equal(q.astype(np.float32).astype(np.float64), q), name
        assert F.exact_pair(P, Q) == hit == F.exact_pair(Q, P), name
        assert F.exact_envelope(P, Q) == env, name
        assert env or not hit, name
    kinds = {(hit, env) for _, _, _, hit, env in pairs}
    assert kinds == {(True, True), (False, True), (False, False)}
    names = " | ".join(n for n, *_ in pairs)
    for word in ("overlapping", "inside", "corner to corner", "corner to edge", "edge to edge", "apart by 2^-4", "diamonds offset", "reversed winding",
                 "exchanged"):
        assert word in names, word


def test_exact_check_on_hand_cases():
    """The independent check itself, on pairs decided by hand."""
    sq = [(0, 0), (2, 0), (2, 2), (0, 2)]
    assert F.exact_pair(sq, [(1, 1), (3, 1), (3, 3), (1, 3)])                       # overlap
    assert F.exact_pair(sq, [(2, 2), (3, 2), (3, 3), (2, 3)])                       # one shared corner
    assert not F.exact_pair(sq, [(2.0625, 0), (3, 0), (3, 2), (2.0625, 2)])         # a gap of 1 / 16
    assert F.exact_pair([(0, 0), (8, 0), (8, 8), (0, 8)], [(3, 3), (4, 3), (4, 4), (3, 4)])      # containment: no edge meets an edge
    assert not F.exact_pair([(1, 0), (0, 1), (-1, 0), (0, -1)], [(2.25, 1.25), (1.25, 2.25), (0.25, 1.25), (1.25, 0.25)])
    assert F.exact_envelope([(1, 0), (0, 1), (-1, 0), (0, -1)], [(2.25, 1.25), (1.25, 2.25), (0.25, 1.25), (1.25, 0.25)])
    assert F.exact_envelope(sq, [(2, 2), (3, 2), (3, 3), (2, 3)]) and not F.exact_envelope(sq, [(2.0625, 0), (3, 0), (3, 2), (2.0625, 2)])


def test_host_statement_equals_the_exact_answer_on_the_known_pairs():
    fp = _fp()
    for name, P, Q, hit, env in F.known_pairs():
        assert bool(fp.pair_collides(P, Q, "footprint")) == hit, name
        assert bool(fp.pair_collides(P, Q, "envelope")) == env, name
        for mode, want in (("footprint", hit), ("envelope", env)):
            flags, first = fp.collision_matrix(P[None, None], Q[None, None], Ts=1, mode=mode)
            assert flags.shape == (1, 1) and flags.dtype == np.bool_ and first.dtype == np.int32
            assert bool(flags[0, 0]) == want and int(first[0, 0]) == (0 if want else -1), (name, mode)


def test_host_statement_shapes_first_actor_and_refusals():
    fp = _fp()
    pairs = {n: (P, Q) for n, P, Q, _, _ in F.known_pairs()}
    P, hit_q = pairs["overlapping"]
    clear_q = pairs["diamonds offset diagonally"][1] + 40.0
    cv = np.full((2, 3, 4, 2), np.nan, dtype=np.float32)      # Tc = 3 > Ts = 1: the rows behind Ts are not read
    cv[:, 0] = P
    ov = np.stack([clear_q, hit_q, hit_q])[:, None]            # two hitting actors: the lower index is reported
    flags, first = fp.collision_matrix(cv, ov, Ts=1)
    assert flags.tolist() == [[True], [True]] and first.tolist() == [[1], [1]]
    for none in (None, np.zeros((0, 1, 4, 2))):
        flags, first = fp.collision_matrix(cv, none, Ts=1)
        assert not flags.any() and (first == -1).all() and flags.shape == (2, 1)
    with pytest.raises(ValueError, match="sat.*known.*envelope.*footprint"):
        fp.collision_matrix(cv, ov, Ts=1, mode="sat")


def test_random_rectangles_footprint_never_exceeds_envelope_and_often_differs():
    """2 000 seeded rectangle pairs at CARLA magnitudes as one (G, Ts, N) problem: footprint <= envelope elementwise, the two differ on more
    than 5 % of the pairs (so the comparison on the device is not vacuous), and both answers occur in both modes."""
    fp = _fp()
    cv, ov = F.random_problem()
    G, Ts, N = F.RANDOM_SHAPE
    assert cv.shape == (G, Ts, 4, 2) and cv.dtype == np.float32 and ov.shape == (N, Ts, 4, 2) and G * Ts * N == 2000
    assert np.abs(ov).max() <= 2010.0 and np.abs(ov[..., 0]).max() > 100.0
    env = fp.pair_collides(cv[:, None], ov[None], "envelope")
    foot = fp.pair_collides(cv[:, None], ov[None], "footprint")
    assert env.shape == (G, N, Ts) and not (foot & ~env).any()
    share = float((env != foot).mean())
    print(f"random rectangles: envelope {env.mean():.3f}, footprint {foot.mean():.3f}, differ {share:.3f}")
    assert share > 0.05 and foot.any() and not env.all()
    # the matrix form says the same
    for mode, pairwise in (("envelope", env), ("footprint", foot)):
        flags, first = fp.collision_matrix(cv, ov, Ts=Ts, mode=mode)
        assert np.array_equal(flags, pairwise.any(1))
        assert np.array_equal(first, np.where(pairwise.any(1), pairwise.argmax(1), -1))


def test_lane_neighbour_scene_envelope_flags_every_candidate_footprint_none():
    """The lane-neighbour scene under the host statement, with the candidates rolled out by the oracle chain: the envelope test flags at least
    one step of every candidate, the footprint test none; the closest the two vehicles come is the lane's width less the two half widths."""
    from oracle import rollout as orl, traj_flags as otf
    fp = _fp()
    traj, entry, actors = F.lane_scene()
    x, y, h = F.LANE_POSE
    gpos, ghead = orl.to_global(traj[0][:, :, :40, :], torch.tensor([x, y]), torch.tensor(h))
    ro = orl.Rollout().propagate(gpos, ghead, F.LANE_STATE["speed"], F.LANE_STATE["width"], F.LANE_STATE["length"])
    other = otf.get_other_vehicle_rollout(num_future_frames=40, near_lane_change=True, bbox_inflation_ratio=1.1, **actors)
    cv = ro["vertices"].numpy().astype(np.float32)
    assert cv.shape == (12, 80, 4, 2) and other.shape == (1, 40, 4, 2)
    env, _ = fp.collision_matrix(cv, other, Ts=40, mode="envelope")
    foot, first = fp.collision_matrix(cv, other, Ts=40, mode="footprint")
    assert env.any(1).all() and env[:, 0].all()
    assert not foot.any() and (first == -1).all()
    assert np.array_equal(env, otf.get_collision_matrix(ro["vertices"].numpy(), other))      # the envelope mode is the reference's test
    # the lateral gap: the neighbour's centre line is LANE_WIDTH to the left, half widths 1.0 and 1.0 * 1.1
    left = np.array([-np.sin(h), np.cos(h)])
    gap = ((other[0, :, :, :] @ left).min() - (cv[:, :40] @ left).max())
    print(f"lane scene: envelope flags {env.sum(1).tolist()} steps per candidate; lateral gap {gap:.3f} m")
    assert 1.0 < gap < F.LANE_WIDTH - 2.1 + 0.05
