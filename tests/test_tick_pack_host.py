"""rift_amd/tick_pack.py on the CPU: the blob of a rollout tick and the RiftTickCBV array that points into it.  Every pointer of every
struct is decoded back out of the blob (minus the base address) and compared with the inputs after their casts; what no pointer covers
has to be zero padding of less than 16 bytes; the blocks lie in the order float64 | float32 | int32 | pad | uint8; centre states and masks
are 16-byte aligned from the blob's start, actor blocks 8-byte, line lengths 4-byte.  The device side of the same call is
tests/test_host_rlft.py (fused tick against the per-CBV chain), tests/test_gpu_eval_params.py and tests/test_gpu_drivable_map.py."""
import ast

import numpy as np
import pytest

from rift_amd import tick_pack
from rift_amd._abi import RiftTickCBV

BASE = 0x7F3A00001000          # a made-up, 16-byte aligned device address
ACTOR_KEYS = {"steer": 1, "throttle": 1, "brake": 1, "speed": 1, "location": 3, "yaw_deg": 1, "extent": 2}


def _actors(g, N):
    return {k: (g.normal(size=(N, w)) if w > 1 else g.normal(size=N)) for k, w in ACTOR_KEYS.items()}


def _entry(seed, batch_index, points, n_actors=None, mask=None, raster=None, pose=None):
    """One entry of float64 readings (so that the float32 casts show): lines of `points` points, n_actors None / 0 (a dict of empty
    arrays) / N, mask None / (H, W)."""
    g = np.random.default_rng(seed)
    v = {"batch_index": batch_index, "center_state": tuple(g.normal(size=6) * 10),
         "ref_pos": [g.normal(size=(n, 2)) * 100 for n in points], "ref_angle": [g.uniform(-3, 3, size=n) for n in points],
         "actors": None if n_actors is None else _actors(g, n_actors), "off_road": None, "raster": raster, "pose": pose}
    if mask is not None:
        v["off_road"] = ((g.random(mask) < 0.5).astype(np.uint8), tuple(g.normal(size=3)))
    return v


ONE_POINT = lambda b=0: _entry(1, b, (1,))                                        # noqa: E731  6 + 2 + 1 = 9 floats: three floats of pad
ODD = lambda b=0: _entry(2, b, (5, 1, 7), n_actors=2, mask=(5, 7))                # noqa: E731  69 floats and a 35-byte mask: both pads
NO_ACTORS = lambda b=0: _entry(3, b, (2, 3), n_actors=0)                          # noqa: E731
MASK16 = lambda b=0: _entry(4, b, (4,), mask=(4, 4))                              # noqa: E731  16 bytes: no pad behind the mask
MAP = lambda b=0: _entry(5, b, (3, 2), n_actors=1, raster=(200, 300), pose=(1.5, -2.5, 0.25))      # noqa: E731
CASES = {"one_point": [ONE_POINT()], "odd_sizes": [ODD()], "zero_length_actors": [NO_ACTORS()], "mask_16_bytes": [MASK16()], "map_entry": [MAP()],
         "all_in_one_tick": [ODD(3), ONE_POINT(0), NO_ACTORS(4), MASK16(1), MAP(2), ODD(5)]}


def _expected(v):
    """What the CBV's pointers must lead to, from the entry alone."""
    R, Pmax = len(v["ref_pos"]), max(len(p) for p in v["ref_pos"])
    rp, ra = np.zeros((R, Pmax, 2), np.float32), np.zeros((R, Pmax), np.float32)
    for r, (p, a) in enumerate(zip(v["ref_pos"], v["ref_angle"])):
        rp[r, :len(p)], ra[r, :len(p)] = p.astype(np.float32), a.astype(np.float32)
    want = {"R": R, "Pmax": Pmax, "center_state": np.asarray(v["center_state"]).astype(np.float32), "ref_pos": rp.reshape(-1),
            "ref_angle": ra.reshape(-1), "ref_len": np.array([len(p) for p in v["ref_pos"]], np.int32), "actors": None, "off_road_mask": None,
            "n_actors": 0, "H": 0, "W": 0, "pose": (0.0, 0.0, 0.0)}
    a = v["actors"]
    if a is not None and len(a["steer"]):
        want["n_actors"] = len(a["steer"])
        want["actors"] = np.concatenate([np.stack([a["steer"], a["throttle"], a["brake"]], -1).reshape(-1), a["speed"], a["location"].reshape(-1),
                                         a["yaw_deg"], a["extent"].reshape(-1)]).astype(np.float64)
    if v["off_road"] is not None:
        mask, pose = v["off_road"]
        want.update(off_road_mask=mask.reshape(-1), H=mask.shape[0], W=mask.shape[1], pose=tuple(float(x) for x in pose))
    elif v["raster"] is not None:
        want.update(H=v["raster"][0], W=v["raster"][1], pose=tuple(float(x) for x in v["pose"]))
    return want


@pytest.mark.parametrize("case", list(CASES))
def test_every_pointer_leads_back_to_the_inputs(case):
    cbvs = CASES[case]
    blob, layout = tick_pack.pack_tick(cbvs)
    arr = tick_pack.fill_tick_cbvs(layout, BASE)
    assert blob.dtype == np.uint8 and blob.ndim == 1 and len(arr) == len(cbvs) and isinstance(arr[0], RiftTickCBV)
    claimed = np.zeros(blob.size, dtype=bool)
    spans = {np.float64: [], np.float32: [], np.int32: [], np.uint8: []}

    def read(address, want, align):
        at = address - BASE
        assert 0 <= at and at + want.nbytes <= blob.size and at % align == 0, (at, align)
        assert not claimed[at:at + want.nbytes].any()                     # no two pieces overlap
        claimed[at:at + want.nbytes] = True
        spans[want.dtype.type].append((at, at + want.nbytes))
        assert blob[at:at + want.nbytes].tobytes() == want.tobytes()      # bit for bit, the zeros behind a short line included

    for t, v in zip(arr, cbvs):
        want = _expected(v)
        assert (t.batch_index, t.R, t.Pmax, t.n_actors, t.H, t.W) == (v["batch_index"], want["R"], want["Pmax"], want["n_actors"], want["H"], want["W"])
        assert tuple(t.pose) == want["pose"]
        read(t.center_state, want["center_state"], 16)
        read(t.ref_pos, want["ref_pos"], 4)
        read(t.ref_angle, want["ref_angle"], 4)
        read(t.ref_len, want["ref_len"], 4)
        for name, align in (("actors", 8), ("off_road_mask", 16)):
            if want[name] is None:
                assert getattr(t, name) is None                           # NULL
            else:
                read(getattr(t, name), want[name], align)
    assert not blob[~claimed].any()                                       # padding is zero ...
    free = np.flatnonzero(~claimed)
    assert all(len(run) < 16 for run in np.split(free, np.flatnonzero(np.diff(free) > 1) + 1))      # ... and never a whole 16 bytes
    order = [spans[k] for k in (np.float64, np.float32, np.int32, np.uint8) if spans[k]]
    for before, after in zip(order, order[1:]):                           # float64 | float32 | int32 | (pad) | uint8
        assert max(e for _, e in before) <= min(s for s, _ in after)
    if spans[np.uint8]:
        assert min(s for s, _ in spans[np.uint8]) - max(e for _, e in spans[np.int32]) < 16


def test_refusals():
    v = MAP()
    v["pose"] = None
    with pytest.raises(ValueError, match=r"group_advantage_tick: an entry with 'raster' needs 'pose' \(x, y, heading of the footprint centre\)"):
        tick_pack.pack_tick([ONE_POINT(), v])
    v = ODD()
    v["actors"]["speed"] = v["actors"]["speed"][:1]
    with pytest.raises(AssertionError, match="per-actor arrays of different lengths"):
        tick_pack.pack_tick([v])


def test_pad_ref_lines():
    g = np.random.default_rng(7)
    pos, ang = [g.normal(size=(n, 2)) for n in (2, 4, 1)], [g.normal(size=n) for n in (2, 4, 1)]
    rp, ra, ref_len = tick_pack.pad_ref_lines(pos, ang)
    assert (rp.shape, ra.shape, rp.dtype, ra.dtype, ref_len.dtype) == ((3, 4, 2), (3, 4), np.float32, np.float32, np.int32)
    assert ref_len.tolist() == [2, 4, 1]
    for r, n in enumerate((2, 4, 1)):
        assert rp[r, :n].tobytes() == pos[r].astype(np.float32).tobytes() and ra[r, :n].tobytes() == ang[r].astype(np.float32).tobytes()
        assert not rp[r, n:].any() and not ra[r, n:].any()
    rp, ra, ref_len = tick_pack.pad_ref_lines([np.ones((1, 2))], [np.ones(1)])          # one line, one point
    assert rp.shape == (1, 1, 2) and ra.shape == (1, 1) and ref_len.tolist() == [1]


def test_actor_block():
    import torch
    a = _actors(np.random.default_rng(8), 3)
    N, block = tick_pack.actor_block(dict(a, speed=torch.from_numpy(a["speed"]).float(), brake=[1, 0, 1]))      # a tensor, a list
    want = np.concatenate([np.stack([a["steer"], a["throttle"], [1.0, 0.0, 1.0]], -1).reshape(-1), a["speed"].astype(np.float32).astype(np.float64),
                           a["location"].reshape(-1), a["yaw_deg"], a["extent"].reshape(-1)])
    assert N == 3 and block.dtype == np.float64 and block.tobytes() == want.tobytes()
    assert tick_pack.actor_block(_actors(np.random.default_rng(8), 0)) == (0, None)
    with pytest.raises(AssertionError, match="per-actor arrays of different lengths"):
        tick_pack.actor_block(dict(a, extent=a["extent"][:2]))


def test_the_module_needs_neither_torch_nor_the_library():
    tree = ast.parse(open(tick_pack.__file__).read())
    names = {n.module if isinstance(n, ast.ImportFrom) else a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))
             for a in n.names}
    assert names == {"collections", "numpy", "rift_amd._abi"}
