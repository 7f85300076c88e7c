"""DropPath grouping of the history encoder (nat_l0w.h: nat_group_body; nat_l1w.h, nat_l2w.hip): in a train-mode forward with drops NAT
levels 1 and 2 take their sequences from two lists sorted by DropPath pattern inside the position classes seq % 4 / seq % 3, and a
half-block that DropPath drops for a whole level-1 tile / a whole level-2 round is not computed.  Every decision is a pure function of
(seed, stream, seq), every buffer stays indexed by seq and a sequence keeps its lane rows, so the grouped forward must equal the
ungrouped one EXACTLY: torch.equal against an engine made with RIFT_NO_SKIP=1 (rank order, everything computed) on the same state dict.

The restatement below (hash32 / uniform01 of lanes.h, the Gray-order key, the tiles and rounds) picks the seeds, predicts the lists'
properties and the skip counters of the diagnostic library.  Level 2 deals a small launch wave-major (a workgroup's round is one tile per
wave, tiles G apart); RIFT_NAT_GRID=8 makes the 12-scene case round-major -- 32 rounds of eight consecutive tiles, four per workgroup -- as
a chip-filling batch runs it.  Needs a real MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

from rift_amd import synthetic as syn
from tests import helpers as H
from tests import history_cases as HC
from tests.test_gpu_skip_discarded import _uniform01

pytestmark = pytest.mark.gpu

STREAM = {1: 6, 2: 11}                                        # engine.hip: NAT levels take streams 1, 6, 11 (one + four each)
RATES = {1: (np.float32(0.08), np.float32(0.12)), 2: (np.float32(0.16), np.float32(0.2))}      # engine.hip: NAT_DPR
CLASSES = {1: 4, 2: 3}
GRAY = [i ^ (i >> 1) for i in range(16)]                      # place in the sort order -> pattern
CH = {"x1": (10, 64), "x2": (5, 128), "oc0": (3, 32), "oc1": (3, 64), "oc2": (3, 128)}
DEFAULT_GRID = 256


# ---- the kernels' decisions, keys, tiles and rounds restated ---------------------------------------------------------------------------
def dropped(seed, lv, n):
    """(n, 4) bool: sequence x (block 0 attention, block 0 MLP, block 1 attention, block 1 MLP) dropped at level lv."""
    seq = np.arange(n)
    return np.stack([_uniform01(seed, STREAM[lv] + b, seq) < RATES[lv][b >> 1] for b in range(4)], axis=1)


def gray_key(d):
    pat = (d * np.array([1, 2, 4, 8])).sum(1)
    key = pat ^ (pat >> 1)
    return key ^ (key >> 2)


def live_ranks(cnt):
    n = 3 * max(cnt)
    r = np.arange(n)
    return n, r[(r // 3) < np.asarray(cnt)[r % 3]]


def sorted_classes(seed, lv, cnt):
    """Per position class the Gray keys of its live ranks in sorted order: the key of the t-th entry of a class does not depend on the
    order inside a bucket, and a tile's drop pattern is a function of these keys only."""
    n, live = live_ranks(cnt)
    key = gray_key(dropped(seed, lv, n))
    return [np.sort(key[live[live % CLASSES[lv] == c]]) for c in range(CLASSES[lv])]


def tile_drops(keys, ntiles):
    """(ntiles, 4) bool "dropped for every sequence of the tile" (a hole counts as dropped), (ntiles,) bool "has a sequence"."""
    drop, has = np.ones((ntiles, 4), dtype=bool), np.zeros(ntiles, dtype=bool)
    for k in keys:
        pat = np.array(GRAY)[k]
        m = min(len(k), ntiles)
        for b in range(4):
            drop[:m, b] &= ((pat[:m] >> b) & 1).astype(bool)
        has[:m] = True
    return drop, has


def l2_rounds(ntiles, G):
    """The tiles of every (workgroup, round) of nat_l2w_kernel's dealing, -1 = a wave without a tile."""
    rounds, nrounds = [], (ntiles + 7) // 8
    if ntiles <= 4 * G:
        for b in range(min(G, ntiles)):
            rounds.append([w * G + b if w * G + b < ntiles else -1 for w in range(8)])
    else:
        for r in range(nrounds):
            rounds.append([r * 8 + w if r * 8 + w < ntiles else -1 for w in range(8)])
    return rounds


def predicted_skips(seed, cnt, nA, grid):
    """The eight counters: level 1's skipped (tile, block, branch), level 2's skipped (workgroup round, block, branch); with them how many
    of those tiles / rounds hold a sequence."""
    n = 3 * max(cnt)
    d1, has1 = tile_drops(sorted_classes(seed, 1, cnt), (n + 3) // 4)
    d2, has2 = tile_drops(sorted_classes(seed, 2, cnt), n // 3)
    G = min(-(-nA // 3), grid)
    r2 = np.zeros(4, dtype=int)
    real2 = np.zeros(4, dtype=int)
    for tiles in l2_rounds(n // 3, G):
        t = [x for x in tiles if x >= 0]
        r2 += d2[t].all(0)
        real2 += d2[t].all(0) & has2[t].any()
    return np.concatenate([d1.sum(0), r2]), np.concatenate([(d1 & has1[:, None]).sum(0), real2])


def pick_seed(cnt, nA, grid, start=1):
    for seed in range(start, 200000):
        if (predicted_skips(seed, cnt, nA, grid)[1] >= 1).all():
            return seed
    raise AssertionError("no seed with a wholly dropped tile and round for every branch")


# ---- engines ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    made = {}
    switches = ("RIFT_NO_SKIP", "RIFT_NAT_GROUP", "RIFT_NAT_GRID")

    def get(name):
        if name in made:
            return made[name]
        env, variant = {"group": ({}, ""), "group-grid8": ({"RIFT_NAT_GRID": "8"}, ""), "noskip": ({"RIFT_NO_SKIP": "1"}, ""),
                        "noskip-grid8": ({"RIFT_NO_SKIP": "1", "RIFT_NAT_GRID": "8"}, ""),
                        "group0": ({"RIFT_NAT_GROUP": "0"}, ""), "stats": ({}, "stats"), "stats-grid8": ({"RIFT_NAT_GRID": "8"}, "stats")}[name]
        old = {k: os.environ.pop(k, None) for k in switches}
        os.environ.update(env)
        try:
            eng = _ffi.Engine("cuda:0", variant=variant)      # (the switches are read when the context is made)
        finally:
            for k in switches:
                os.environ.pop(k, None)
                if old[k] is not None:
                    os.environ[k] = old[k]
        eng.load_state_dict({k: v.clone() for k, v in H.weights().items()})
        made[name] = eng
        return eng

    yield get
    for e in made.values():
        e.close()


_d = {}


def batch(name):
    if name not in _d:
        agents = {"twelve": [64] * 12, "five": [5], "seven-and-64": [7, 64]}[name]
        scenes = [syn.make_scene(7700 + i, num_agents=a, num_polygons=8, r_min=1, r_max=4) for i, a in enumerate(agents)]
        data = syn.collate_scenes(scenes)["cur_pluto_feature_torch"]
        if name == "twelve":
            data["agent"]["valid_mask"][:, :, 10] = True      # every slot an agent: 12 x 63 = 756 sequences, 252 level-2 tiles
        _d[name] = (data, HC.ranking(data)[2], data["agent"]["position"].shape[0] * data["agent"]["position"].shape[1])
    return _d[name]


def run(eng, data, cnt, **kw):
    """The forward's `probability` and the history taps: rank-ordered rows of the live ranks only (the others nobody writes)."""
    out = eng.forward(data, bn_update=False, **kw)
    torch.cuda.synchronize()
    assert eng.tap("nat_cnt").cpu().view(torch.int32).tolist()[:3] == cnt
    n, live = live_ranks(cnt)
    got = {"f9": eng.tap("nat_f9").cpu(),
           "out": eng.tap("nat_out").cpu().view(-1, 128)[HC.ranking(data)[0]].clone()}      # (rows of the history slots: the others nobody writes)
    for t, shape in CH.items():
        raw = eng.tap("nat_" + t).cpu()
        if t.startswith("oc"):
            raw = raw.view(torch.int16)                       # (the 16-bit operand words the FPN tail receives)
        got[t] = raw.view(-1, *shape)[:n][live].clone()
    got["probability"] = out["probability"].cpu().clone()
    return got


def same(a, b, what):
    assert a.keys() == b.keys()
    for t in a:
        assert torch.isfinite(a[t].float()).all(), (what, t)
        assert torch.equal(a[t], b[t]), f"{what}: {t} differs in {int((a[t] != b[t]).sum())} words"


def lists(eng):
    return eng.tap("nat_perm1").cpu().view(torch.int32).numpy(), eng.tap("nat_perm2").cpu().view(torch.int32).numpy()


def check_list(perm, lv, seed, cnt):
    """A permutation of exactly the live ranks; entry k of class k % C; Gray keys non-decreasing inside a class; holes last."""
    C = CLASSES[lv]
    n, live = live_ranks(cnt)
    key = gray_key(dropped(seed, lv, n))
    assert perm.size % C == 0
    assert sorted(perm[perm >= 0].tolist()) == live.tolist()
    assert set(perm[perm < 0].tolist()) <= {-1}
    for c in range(C):
        col = perm[c::C]
        m = int((col >= 0).sum())
        assert (col[:m] >= 0).all() and (col[m:] == -1).all(), (lv, c, "holes come last")
        assert (col[:m] % C == c).all(), (lv, c)
        assert (np.diff(key[col[:m]]) >= 0).all(), (lv, c, "sorted by Gray key")


# ---- tests --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [DEFAULT_GRID, 8])
def test_grouped_equals_ungrouped(engines, grid):
    """12 scenes x 64 agent slots.  The seed: the first under which the sorted order holds a wholly dropped level-1 tile and a wholly dropped
    level-2 round (tiles / rounds that hold sequences) for each of the four branches of either level."""
    data, cnt, nA = batch("twelve")
    assert cnt == [252, 252, 252]
    assert len(l2_rounds(252, grid)) == (32 if grid == 8 else 252), "round-major: 32 rounds of eight tiles; wave-major: one tile a workgroup"
    seed = pick_seed(cnt, nA, grid)
    skips, real = predicted_skips(seed, cnt, nA, grid)
    print(f"    grid {grid}: seed {seed}, predicted skips {skips.tolist()} (with sequences: {real.tolist()})")
    assert (real >= 1).all()
    # (the reference on the same grid: the switch also sizes the PointsEncoder's persistent launch, whose train-mode BatchNorm sums are
    # added up per workgroup)
    eng, ref = (engines("group"), engines("noskip")) if grid == DEFAULT_GRID else (engines("group-grid8"), engines("noskip-grid8"))
    a = run(eng, data, cnt, train=True, seed=seed)
    p1, p2 = lists(eng)
    check_list(p1, 1, seed, cnt)
    check_list(p2, 2, seed, cnt)
    b = run(ref, data, cnt, train=True, seed=seed)
    same(a, b, f"grouped against RIFT_NO_SKIP=1, seed {seed}")
    other = run(eng, data, cnt, train=True, seed=seed + 1)
    assert not torch.equal(other["oc2"], a["oc2"]) and not torch.equal(other["oc1"], a["oc1"])      # (the drops are on: another seed, other rows)
    same(other, run(ref, data, cnt, train=True, seed=seed + 1), f"seed {seed + 1}")


@pytest.mark.parametrize("name", ["five", "seven-and-64"])
def test_edges(engines, name):
    """One scene of 5 agent slots: less than one round, the lists mostly holes.  Scenes of 7 and 64 slots: unequal class counts, a partial
    last round, bucket edges inside tiles."""
    data, cnt, nA = batch(name)
    assert sum(cnt) >= 1
    if name == "five":
        assert sum(cnt) <= 4
    else:
        assert len(set(cnt)) > 1 and max(cnt) % 8 != 0
    for seed in (3, 4, 5):
        a = run(engines("group"), data, cnt, train=True, seed=seed)
        p1, p2 = lists(engines("group"))
        check_list(p1, 1, seed, cnt)
        check_list(p2, 2, seed, cnt)
        same(a, run(engines("noskip"), data, cnt, train=True, seed=seed), f"{name}, seed {seed}")


@pytest.mark.parametrize("grid", [DEFAULT_GRID, 8])
def test_skips_happen_and_decisions_are_the_restated_ones(engines, grid):
    """The diagnostic library: the eight skip counters equal the restatement's, and the per-sequence decisions recorded under `seq` are the
    restated ones (every live sequence recorded, the lane rows of a sequence agreeing)."""
    data, cnt, nA = batch("twelve")
    seed = pick_seed(cnt, nA, grid)
    want = predicted_skips(seed, cnt, nA, grid)[0]
    eng = engines("stats" if grid == DEFAULT_GRID else "stats-grid8")
    a = run(eng, data, cnt, train=True, seed=seed)
    got = eng.tap("nat_skip").cpu().view(torch.int32).numpy()
    print(f"    grid {grid}: seed {seed}, skipped {got.tolist()}, predicted {want.tolist()}")
    assert got.tolist() == want.tolist()
    assert (got >= 1).all()
    bs = data["agent"]["position"].shape[0]
    nmax = max(nA, bs * 6)
    kept = eng.tap("drop_any").cpu().view(torch.int32).numpy().view(np.uint32).reshape(21, nmax)
    allk = eng.tap("drop_all").cpu().view(torch.int32).numpy().view(np.uint32).reshape(21, nmax)
    seen = eng.tap("drop_cnt").cpu().view(torch.int32).numpy().view(np.uint32).reshape(21, nmax)
    n, live = live_ranks(cnt)
    for lv in (1, 2):
        d = dropped(seed, lv, n)
        for b in range(4):
            site = lv * 4 + b
            assert (seen[site, live] > 0).all(), (lv, b)
            assert np.array_equal(kept[site, live] == 0, d[live, b]), (lv, b)
            assert np.array_equal(allk[site, live] == 0, d[live, b]), (lv, b)
    assert all(torch.isfinite(v.float()).all() for v in a.values())


def test_other_paths_are_the_ungrouped_ones(engines):
    """Eval mode, a train forward with no_drop, and RIFT_NAT_GROUP=0: the launches and the outputs of the RIFT_NO_SKIP=1 engine."""
    data, cnt, nA = batch("seven-and-64")

    def profiled(eng, **kw):
        run(eng, data, cnt, **kw)                         # (an engine's first forward of a mode carries one-time launches of its own)
        eng.prof_enable(True)
        got = run(eng, data, cnt, **kw)
        rep = eng.prof_report()
        eng.prof_enable(False)
        return got, {k: v["count"] for k, v in rep.items()}

    for who, kw in (("group", dict(train=False)), ("group", dict(train=True, no_drop=True, seed=9)), ("group0", dict(train=True, seed=9))):
        a, la = profiled(engines(who), **kw)
        b, lb = profiled(engines("noskip"), **kw)
        assert la == lb, (who, kw)
        assert "nat_l1w_kernel" in la and "nat_l2w_kernel" in la
        same(a, b, f"{who} {kw}")
