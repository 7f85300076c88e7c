"""Work the step discards is not computed (round 8): the scene encoder skips a branch DropPath drops for its scene (enc_fused.h), the planning
decoder skips m2m on a padded reference line and, in a forward without the trajectory heads, the whole last-layer reference-line tiling of
such a line (dec_w.hip).  RIFT_NO_SKIP=1 keeps the earlier path -- compute, then multiply by zero / overwrite with zeros -- in the same
binary.  Every random decision is a pure function of (seed, stream, index) and the decoder's dropout streams are stepped past the draws a
skipped sub-block would have made (tests/test_lcg_jump.py), so the two paths must agree EXACTLY: torch.equal throughout.

Zero rows behind the last-layer skip: the rows the decoder kernel writes are its output array (tap `dec3`); the tap named `q_final` is
cat_x_proj of them, whose bias and ego-token half leave no row zero.  So the zero rows are asserted on `dec3`, and `q_final` must hold, on
every padded line of a scene, the one row cat_x_proj makes of a zero query (all of them identical, and finite)."""
import numpy as np
import pytest
import torch

from rift_amd import synthetic as syn
from tests import helpers as H

pytestmark = pytest.mark.gpu

ENC_STREAM = 17                 # engine.hip: NAT levels take streams 1, 6, 11 (one + four each), the ego token's state dropout 16, the scene encoder the next
ENC_RATES = [np.float32(0.0), np.float32(0.2) / np.float32(3.0), np.float32(0.4) / np.float32(3.0), np.float32(0.2)]     # engine.hip: edpr


# ---- common.h restated: hash32 / uniform01 -------------------------------------------------------------------------------------------
def _u32(x):
    return x & np.uint64(0xFFFFFFFF)


def _hash32(seed, stream, idx):
    seed, stream, idx = np.uint64(seed), np.uint64(stream), np.asarray(idx, dtype=np.uint64)

    def mix(x):
        x = x ^ (x >> np.uint64(16)); x = _u32(x * np.uint64(0x7FEB352D))
        x = x ^ (x >> np.uint64(15)); x = _u32(x * np.uint64(0x846CA68B))
        return x ^ (x >> np.uint64(16))

    x = _u32(_u32(idx * np.uint64(0x9E3779B1)) + (seed ^ _u32(stream * np.uint64(0x85EBCA6B))))
    x = mix(x)
    x = _u32(x + _u32(seed * np.uint64(0xC2B2AE35)) + stream)
    return mix(x)


def _uniform01(seed, stream, idx):
    return (_hash32(seed, stream, idx) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _enc_dropped(seed, bs):
    """(4 layers, 2 branches, bs) bool: the branches enc_fused_body drops (uniform01(seed, stream + 2 layer + branch, scene) < rate)."""
    d = np.zeros((4, 2, bs), dtype=bool)
    for li in range(1, 4):
        for br in range(2):
            d[li, br] = _uniform01(seed, ENC_STREAM + 2 * li + br, np.arange(bs)) < ENC_RATES[li]
    return d


def _covered(d):
    return d[1:].any(-1).all() and (d[1:, 0] & d[1:, 1]).any()


def _pick_seed(bs):
    """The first seed under which each of the six droppable branches is dropped for some scene and some scene loses both branches of a layer."""
    for seed in range(1, 200000):
        if _covered(_enc_dropped(seed, bs)):
            return seed
    raise AssertionError("no seed with full coverage")


# ---- two engines on one state dict: the skipping path and RIFT_NO_SKIP=1 ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    sd = H.weights()
    made = {}
    with pytest.MonkeyPatch.context() as mp:
        for name, val in (("skip", None), ("noskip", "1")):
            if val is None:
                mp.delenv("RIFT_NO_SKIP", raising=False)
            else:
                mp.setenv("RIFT_NO_SKIP", val)
            made[name] = _ffi.Engine("cuda:0")               # (the switches are read when the context is made)
            made[name].load_state_dict({k: v.clone() for k, v in sd.items()})
    yield made
    for e in made.values():
        e.close()


def _run(eng, data, taps, **kw):
    out = eng.forward(data, bn_update=False, **kw)
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().clone() for k, v in out.items()}
    for t in taps:
        got[t] = eng.tap(t).cpu().clone()
    return got


def _both(engines, data, taps, **kw):
    return _run(engines["skip"], data, taps, **kw), _run(engines["noskip"], data, taps, **kw)


def _line_masks(data):
    rv = data["reference_line"]["valid_mask"].any(-1)       # (bs, R)
    return rv, ~rv


# ---- encoder ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agents,polygons,bs,kernel", [(12, 4, 24, "enc_fused_kernel"), (49, 60, 8, "enc_fused112_kernel")])
def test_encoder_skips_dropped_branches(engines, agents, polygons, bs, kernel):
    """96-row layout: 16 token slots, one row tile of valid tokens, the 5-tile body; 112-row layout: 109 slots.  The seed comes from the
    restatement of the kernel's DropPath decisions above: every droppable branch dropped for some scene, one scene with a whole layer dropped."""
    seed = _pick_seed(bs)
    d = _enc_dropped(seed, bs)
    assert d[1:].any(-1).all(), "each of the six droppable branches is dropped for at least one scene"
    assert (d[1:, 0] & d[1:, 1]).any(), "one scene loses both branches of a layer"
    assert not d[0].any()
    scenes = [syn.make_scene(7100 + i, num_agents=agents, num_polygons=polygons, r_min=1, r_max=4) for i in range(bs)]
    data = syn.collate_scenes(scenes)["cur_pluto_feature_torch"]
    assert data["agent"]["position"].shape[1] + data["map"]["point_position"].shape[1] == agents + polygons
    eng = engines["skip"]
    eng.prof_enable(True)
    a = _run(eng, data, ("enc_out",), train=True, seed=seed)
    ran = eng.prof_report()
    eng.prof_enable(False)
    assert kernel in ran
    b = _run(engines["noskip"], data, ("enc_out",), train=True, seed=seed)
    assert torch.isfinite(a["enc_out"]).all()
    assert torch.equal(a["enc_out"], b["enc_out"])
    assert torch.equal(a["probability"], b["probability"])
    other = _run(eng, data, ("enc_out",), train=True, seed=seed + 1)
    assert not torch.equal(other["enc_out"], a["enc_out"])      # (the drops are on: another seed, other rows)


def test_encoder_decisions_are_the_restated_ones():
    """The restatement the coverage above rests on, against the decisions the kernel records in the diagnostic library (dropstats.h)."""
    from rift_amd import _ffi
    bs = 24
    seed = _pick_seed(bs)
    d = _enc_dropped(seed, bs)
    eng = _ffi.Engine("cuda:0", variant="stats")
    eng.load_state_dict({k: v.clone() for k, v in H.weights().items()})
    data = syn.collate_scenes([syn.make_scene(7100 + i, num_agents=12, num_polygons=4, r_min=1, r_max=4) for i in range(bs)])["cur_pluto_feature_torch"]
    eng.forward(data, train=True, seed=seed, bn_update=False)
    torch.cuda.synchronize()
    nmax = max(bs * 12, bs * 6)
    kept = eng.tap("drop_any").view(torch.int32).cpu().numpy().view(np.uint32).reshape(21, nmax)
    eng.close()
    for li in range(1, 4):
        for br in range(2):
            assert np.array_equal(kept[12 + li * 2 + br, :bs] == 0, d[li, br]), (li, br)


# ---- decoder ------------------------------------------------------------------------------------------------------------------------------
def _decoder_case(engines, scenes):
    data = syn.collate_scenes(scenes)["cur_pluto_feature_torch"]
    rv, rp = _line_masks(data)
    assert rp.any(), "the batch has padded reference lines"
    bs, R = rv.shape
    for kw in (dict(train=True, seed=23), dict(train=False)):
        a, b = _both(engines, data, ("q_final", "dec3"), **kw)
        qa, qb = a["q_final"].view(bs, R, 12, 128), b["q_final"].view(bs, R, 12, 128)
        assert torch.isfinite(qa[rv]).all()
        assert torch.equal(qa[rv], qb[rv]), kw
        assert torch.equal(a["dec3"].view(bs, R, 12, 128)[rv], b["dec3"].view(bs, R, 12, 128)[rv]), kw
        assert torch.equal(a["probability"], b["probability"]), kw
        assert (a["probability"][rp] == -1e6).all()
    return data, rv, rp


def test_decoder_standard_shape_every_valid_line_count(engines):
    """12 scenes, six line slots, valid-line counts 1 .. 6 twice over: every wave of the reference-line tiling is a padded tile in some scene."""
    scenes = [syn.make_scene(7300 + i, num_agents=24, num_polygons=10, r_min=1 + i % 6, r_max=1 + i % 6) for i in range(12)]
    data, rv, rp = _decoder_case(engines, scenes)
    assert rv.shape == (12, 6) and sorted(set(rv.sum(-1).tolist())) == [1, 2, 3, 4, 5, 6]


def test_decoder_mid_shape(engines):
    """97 .. 128 token slots, R <= 8: the eight-key-tile kernel behind the 112-row encoder."""
    scenes = [syn.make_scene(7400 + i, num_agents=49, num_polygons=60, r_min=1 + (2 * i) % 7, r_max=1 + (2 * i) % 7) for i in range(5)]
    data, rv, rp = _decoder_case(engines, scenes)
    n = data["agent"]["position"].shape[1] + data["map"]["point_position"].shape[1]
    assert 97 <= n <= 128 and rv.shape[1] <= 8


def test_decoder_dense_shape(engines):
    """R = 9 .. 12, three scenes: rounds of eight tiles, the second round's tiles are the lines 8 .. 11."""
    scenes = [syn.make_scene(7500 + i, num_agents=24, num_polygons=10, r_min=r, r_max=r) for i, r in enumerate((9, 10, 12))]
    data, rv, rp = _decoder_case(engines, scenes)
    assert rv.shape == (3, 12)


@pytest.mark.parametrize("train", [False, True])
def test_last_layer_skip(engines, train):
    """Without the trajectory heads the rows of padded lines leave the decoder as zeros (nobody reads them: the policy head writes -1e6 there,
    the objectives mask them); everything else equals the RIFT_NO_SKIP run.  With the heads the forward is the RIFT_NO_SKIP run on every row."""
    scenes = [syn.make_scene(7300 + i, num_agents=24, num_polygons=10, r_min=1 + i % 6, r_max=1 + i % 6) for i in range(12)]
    data = syn.collate_scenes(scenes)["cur_pluto_feature_torch"]
    rv, rp = _line_masks(data)
    bs, R = rv.shape
    kw = dict(train=train, seed=31)
    a, b = _both(engines, data, ("q_final", "dec3"), need_traj=False, **kw)
    da, db = a["dec3"].view(bs, R, 12, 128), b["dec3"].view(bs, R, 12, 128)
    qa, qb = a["q_final"].view(bs, R, 12, 128), b["q_final"].view(bs, R, 12, 128)
    assert torch.equal(a["probability"], b["probability"])
    assert torch.equal(qa[rv], qb[rv]) and torch.equal(da[rv], db[rv])
    assert (da[rp] == 0).all(), "padded lines: zero rows out of the decoder"
    assert db[rp].abs().max() > 0, "(the reference path computes something there)"
    assert torch.isfinite(qa).all()
    for s in range(bs):                                     # cat_x_proj of a zero query: one row per scene, whatever the line and the mode
        rows = qa[s][rp[s]].reshape(-1, 128)
        if rows.shape[0]:
            assert (rows == rows[0]).all()
    a, b = _both(engines, data, ("q_final", "dec3"), need_traj=True, **kw)
    for k in ("probability", "trajectory", "prediction", "ref_free_trajectory", "hidden", "q_final", "dec3"):
        assert torch.equal(a[k], b[k]), k
