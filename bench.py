"""RIFT policy-update benchmark on MI355X (contract: see the task brief / DESIGN.md section "Measurement").

    python bench.py                         # 1 GPU, 200 timed steps
    python bench.py --gpus N ...            # N > 1 from a plain shell: runs itself under torch.distributed.run (one rank per GPU, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --full ...              # + every companion figure (see below); the --no-* switches drop single companions of a --full run
    python bench.py --dump-outputs DIR ...  # + what the last timed step computed, as DIR/<name>.npy (loss, probability, pi_head and its gradients)

A plain run builds the headline leg, brings the device's clocks up with a throwaway leg of 200 update steps (what the companion legs used
to do in front of the headline), runs W warm-up and K timed steps and prints the JSON line: nothing else.  `--full` adds the companion
figures: the same steps with every output computed (all_outputs) and 200 of them in one region (steady_state), the full 16-epoch update, the
roofline leg (per-kernel times + rocprofv3 counter child runs), the fp16 / fp32 legs and the precision contract, the end-to-end update, the
CARLA-shaped step, the rollout tick, the CPU baseline and, with N > 1, the other scaling mode.

One *step* = one policy-update step of the reference's RIFT trainer on a 256-scene minibatch per GPU:
device-side collation of 256 scenes from the HBM-resident replay arena -> train-mode PlanningModel
forward (dropout / DropPath / state-dropout on, BatchNorm batch statistics) -> RIFT dual-clip loss ->
analytic pi_head backward -> clip_grad_norm_(0.5) -> AdamW.  With N > 1 ranks three RCCL all-reduces per step
(two inside the forward: BatchNorm sums + the r2r quirk's padding rows; one after the backward: gradient sums,
objective sum, valid count) make the sharded step equal the single-process step on the global minibatch.
Workload = BASELINE.json configs[2]/[3]: 4096-scene synthetic replay, 64 agents x 20 polygons x R~U{1..6}
reference lines x 12 modes.

Scaling.  With N > 1 the headline is STRONG scaling, the partition SURVEY.md 8(e) / north_star state: the reference's 256-scene minibatch
(train_batch_size: 256, fine_tuner/rlft/config/datamodule/rift_datamodule.yaml:2) split contiguously over the ranks -- 256 / N scenes per GPU
per step, global batch 256, the reference's 15 optimizer steps per epoch; every rank holds the whole replay.  The same run also times WEAK
scaling (256 scenes per GPU per step, global minibatch 256 N, the replay sharded) and reports it in the `weak` object (`--scaling weak`
makes it the headline instead).  The driver's per-N efficiency is therefore steps/s (N) / steps/s (1) on a FIXED 256-scene step.
Precision.  The headline runs bf16 MFMA operands (BASELINE.json); at N = 1 the `precisions` object carries the same steps in fp16
operands (same kernels built for v_mfma_f32_16x16x32_f16) and in exact fp32 (layer by layer, the reference's `precision: 32`).
"""
import argparse
import glob
import json
import os
import socket
import sys
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before the HIP runtime initialises (rift_amd/__init__.py explains; an explicit setting wins)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver supports dmabuf IPC only: RCCL needs it for any N > 1

import torch  # noqa: E402

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

FLOPS_PER_SCENE = 1.335e9        # reference-equivalent forward FLOPs/scene at (A=64, Mp=20, R=4), every output computed
FLOPS_PER_SCENE_LOSS = 1.285e9   # the loss-necessary subset (no trajectory / prediction / ref-free heads) -- what the headline step executes
PEAK_BF16_TFLOPS = 2500.0        # MI355X dense bf16 / fp16 MFMA peak (MI355X_MICROARCH.md)
BATCH = 256


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(scenes, sd, contract=None):
    """The reference update step restated on the host cores (oracle = PyTorch-CPU fp32 port of the reference algorithm): CPU collate
    (pad_sequence) -> forward (BatchNorm batch stats, drop p=0) -> RIFT loss -> autograd pi_head backward -> clip 0.5 -> AdamW.
    Bounded sample (~25 s): 5 steps at 32 threads (the fastest count measured on the 256-core GPU box: 4 -> 76, 8 -> 117, 16 -> 131,
    32 -> 145, 64 -> 71 scenes/s forward) and 2 steps at the reference's own default of 4 threads (scripts/run.py:133,164)."""
    from oracle import losses, pluto_ref
    from rift_amd import synthetic as syn
    prefix = "planning_decoder.pi_head."

    def run(threads, steps):
        torch.set_num_threads(threads)
        params = {k: sd[prefix + k].clone().requires_grad_(True) for k in losses.PI_KEYS}
        opt = torch.optim.AdamW(list(params.values()), lr=1e-4, weight_decay=1e-5)

        def one_step(chunk):
            batch = syn.collate_scenes(chunk)
            data = batch["cur_pluto_feature_torch"]
            _, _, taps = pluto_ref.planning_model_forward(sd, data, train_bn=True, need_traj=True, want_taps=True)
            r_pad = ~data["reference_line"]["valid_mask"].any(-1)
            live = dict(sd)
            live.update({prefix + k: v for k, v in params.items()})
            pi = pluto_ref.mlp_layer(taps["q_final"], pluto_ref.SD(live, prefix)).squeeze(-1)
            prob = pi.masked_fill(r_pad.unsqueeze(-1), -1e6)
            loss = losses.rift_loss(prob, r_pad, batch["old_group_logits_torch"], batch["group_advantage_torch"],
                                    batch["group_advantage_mask_torch"])
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(params.values()), 0.5)
            opt.step()

        one_step(scenes[:32])          # warm-up (thread pool, allocator)
        t0 = time.perf_counter()
        n = 0
        for s in range(steps):
            chunk = scenes[s * BATCH:(s + 1) * BATCH]
            if len(chunk) < BATCH:
                break
            one_step(chunk)
            n += 1
        dt = time.perf_counter() - t0
        return n, dt

    hw = os.cpu_count() or 1
    threads = min(32, hw)
    n, dt = run(threads, 5)
    n4, dt4 = run(min(4, hw), 2)
    contract_oracle = None
    if contract is not None:
        # the precision contract's checker side (main(): precision_contract): the four objectives of the parity test's 256-scene batch from the
        # oracle, exactly as tests/test_gpu_parity.py::test_benchmark_batch_objectives_in_16bit_modes computes them -- checker only, not timed
        torch.set_num_threads(threads)
        cdata = contract["cur_pluto_feature_torch"]
        _, _, ctaps = pluto_ref.planning_model_forward(sd, cdata, train_bn=True, need_traj=False, want_taps=True)
        c_pad = ~cdata["reference_line"]["valid_mask"].any(-1)
        contract_oracle = {kind: float(losses.pi_head_loss_and_grads(sd, ctaps["q_final"], kind, _clone_tree(contract), c_pad)[0]) for kind in CONTRACT_KINDS}
    return {"contract_oracle": contract_oracle, "value": n * BATCH / dt, "unit": "scenes/s", "cores": threads, "kind": "port",
            "sample": f"{n} update steps x {BATCH} scenes (collate+fwd all outputs+RIFT loss+bwd+clip+AdamW), PyTorch-CPU fp32 oracle, "
                      f"train-mode BatchNorm batch statistics with every drop probability 0 (the GPU step runs dropout / DropPath / "
                      f"state-dropout: the oracle has no RNG work to do), {dt:.1f}s at {threads} threads; {n4} steps, {dt4:.1f}s at 4 threads",
            "steps_per_sec": n / dt,
            "reference_default_4_threads": {"value": n4 * BATCH / dt4, "unit": "scenes/s", "cores": min(4, hw), "steps_per_sec": n4 / dt4},
            "cpu_model": cpu_model_name(), "logical_cpus": hw}


# ---- committed counter tables (profiles/rNN_pmc_*): counters cannot be collected from inside the process, so the roofline object cites the
# newest committed PMC passes of this same command (tools/profile_round.sh) and names the file
def _newest(pattern):
    files = sorted(glob.glob(os.path.join(REPO, "profiles", pattern)))
    return files[-1] if files else None


def pmc_traffic_file():
    return _newest("r*_pmc_traffic.json")


def kernel_of(label):
    """Engine profiler label -> substring of the kernel's name in the rocprofv3 tables (labels ARE kernel names; GEMM labels carry the
    tile variant and, with RIFT_PROF_SHAPES, a shape suffix)."""
    key = label.split(":")[0]
    gemm = {"gemm_bf16_m1n8": "gemm_rows_kernel<true, 1, 8", "gemm_bf16_m4n2": "gemm_rows_kernel<true, 4, 2", "gemm_bf16_m2n6": "gemm_rows_kernel<true, 2, 6",
            "gemm_bf16_m4n4": "gemm_rows_kernel<true, 4, 4", "gemm_fp32_m1n8": "gemm_rows_kernel<false, 1, 8", "gemm_fp32_m4n2": "gemm_rows_kernel<false, 4, 2",
            "gemm_fp32_m2n6": "gemm_rows_kernel<false, 2, 6", "gemm_fp32_m4n4": "gemm_rows_kernel<false, 4, 4"}
    alias = {"pe_stats1_kernel": "pe_stats1"}          # (pe_stats1_kernel / pe_stats1p_kernel share a label)
    return gemm.get(key, alias.get(key, key))


def pmc_traffic(label, path=None):
    """HBM bytes per launch of the kernel behind an engine profiler label, from the committed PMC passes (None if absent)."""
    path = path or pmc_traffic_file()
    if path is None:
        return None
    kern = json.load(open(path))["kernels"]
    key = kernel_of(label)
    hit = [v for k, v in kern.items() if key in k]
    if not hit:
        return None
    n = sum(v["launches"] for v in hit)
    return sum((2.0 * v["fetch_kb"] + v["write_kb"]) * 1024.0 * v["launches"] for v in hit) / max(n, 1)


def pmc_mfma(label, path=None):
    """(executed MFMA FLOPs per launch, MFMA-busy fraction, source) of a kernel from the committed MFMA counter pass, or None."""
    path = path or _newest("r*_pmc_SQ_INSTS_VALU_MFMA_MOPS_BF16.txt")
    if path is None:
        return None
    cols, key = None, kernel_of(label)
    for line in open(path):
        if line.startswith("dispatches"):
            cols = [c.split("/")[0] for c in line.split()]
            continue
        if cols is None or line.startswith("#") or key not in line:
            continue
        vals = line.split(None, len(cols) - 1)
        row = dict(zip(cols[:-1], vals[:-1]))
        try:
            mops = float(row["SQ_INSTS_VALU_MFMA_MOPS_BF16"])
            busy = float(row["SQ_VALU_MFMA_BUSY_CYCLES"]) / (4.0 * float(row["SQ_BUSY_CU_CYCLES"]))
        except (KeyError, ValueError, ZeroDivisionError):
            return None
        return mops * 512.0, busy, os.path.relpath(path, REPO)
    return None


def collect_counters(label, precision):
    """Roofline counters of the kernel behind `label`, collected in THIS run: three short child runs of this file (4 profiled update steps each,
    serial launches like the roofline leg) under `rocprofv3 --kernel-trace --pmc ...` -- one pass per counter group, kernel-trace only, as
    MI355X_MICROARCH.md's rocprofv3 section prescribes (FETCH_SIZE and WRITE_SIZE do not fit one pass) -- read back from the rocpd database.
    Returns None when rocprofv3 is not on the box (the caller then falls back to the committed tables and says so)."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    rp = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rp is None or os.environ.get("RIFT_BENCH_NO_PMC") == "1":
        return None
    key = kernel_of(label)
    passes = [["FETCH_SIZE"], ["WRITE_SIZE"], ["SQ_INSTS_VALU_MFMA_MOPS_BF16", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CU_CYCLES"]]
    got, launches = {}, 0
    env = dict(os.environ, RIFT_TWO_STREAMS="0", RIFT_PIPELINE="0", TMPDIR="/tmp")
    root = tempfile.mkdtemp(prefix="rift_pmc_", dir="/tmp")
    try:
        for i, ctrs in enumerate(passes):
            out = os.path.join(root, f"p{i}")
            cmd = [rp, "--kernel-trace", "--pmc"] + ctrs + ["-d", out, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--steps", "4", "--warmup", "2",
                   "--replay", "512", "--precision", precision, "--full", "--no-cpu-baseline", "--no-roofline", "--no-full-update", "--no-precisions", "--no-carla",
                   "--no-tick", "--no-e2e"]
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=600)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith(".db")]
            if r.returncode != 0 or not dbs:
                sys.stderr.write(f"bench.py: counter pass {ctrs} failed (rc {r.returncode}): {r.stderr[-300:]}\n")
                return None
            con = sqlite3.connect(dbs[0])
            cols = [c[1] for c in con.execute("pragma table_info('counters_collection')")]
            kcol = "kernel_name" if "kernel_name" in cols else "name"
            ncol = "counter_name" if "counter_name" in cols else "pmc_name"
            vcol = "value" if "value" in cols else "counter_value"
            did = "dispatch_id" if "dispatch_id" in cols else None
            q = f"select {kcol}, {ncol}, sum({vcol}), {'count(distinct ' + did + ')' if did else 'count(*)'} from counters_collection group by {kcol}, {ncol}"
            for kname, cname, total, n in con.execute(q):
                if key in kname:
                    got[cname] = got.get(cname, 0.0) + float(total)
                    launches = max(launches, int(n))
            con.close()
    except (subprocess.TimeoutExpired, sqlite3.Error, OSError) as e:
        sys.stderr.write(f"bench.py: counter collection failed: {e}\n")
        return None
    finally:
        shutil.rmtree(root, ignore_errors=True)
    need = ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU_MFMA_MOPS_BF16", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CU_CYCLES")
    if launches == 0 or any(k not in got for k in need):
        sys.stderr.write(f"bench.py: no counters for {label!r} (kernel key {key!r}; got {sorted(got)})\n")
        return None
    # per launch; gfx950: FETCH_SIZE counts 64 B per 128-B request of a wide coalesced read -> x2 (MI355X_MICROARCH.md, HBM); KB -> B
    # (each pass profiles the same launches, so per-pass sums divide by the same count)
    n = float(launches)
    return {"traffic": (2.0 * got["FETCH_SIZE"] + got["WRITE_SIZE"]) * 1024.0 / n, "fetch_kb": got["FETCH_SIZE"] / n, "write_kb": got["WRITE_SIZE"] / n,
            "mfma_flops": got["SQ_INSTS_VALU_MFMA_MOPS_BF16"] * 512.0 / n,
            "mfma_busy_frac": got["SQ_VALU_MFMA_BUSY_CYCLES"] / (4.0 * got["SQ_BUSY_CU_CYCLES"]) if got["SQ_BUSY_CU_CYCLES"] else None,
            "launches_profiled": launches}


CONTRACT_KINDS = ("rift", "grpo", "reinforce", "ppo")


def contract_batch():
    """The 256-scene batch tests/test_gpu_parity.py::test_benchmark_batch_objectives_in_16bit_modes uses (scenes 1000..1255, PPO advantage seed 99)."""
    from rift_amd import synthetic as syn
    batch = syn.collate_scenes([syn.make_scene(1000 + i) for i in range(256)])
    batch["advantage_torch"] = torch.randn(256, generator=torch.Generator().manual_seed(99))
    return batch


def _clone_tree(t):
    return {k: _clone_tree(v) for k, v in t.items()} if isinstance(t, dict) else (t.clone() if torch.is_tensor(t) else t)


def contract_device_losses(dev, sd, batch, precision):
    """The four objectives of the contract batch on the HIP engine in one compute precision: train-mode forward (BatchNorm batch statistics,
    every drop disabled -- the oracle has no RNG) -> rift_loss_backward -> rift_loss_finalize.  Product path only; no oracle here."""
    from rift_amd import _ffi
    from rift_amd.planning.fine_tuner.rlft.trainer import PI_KEYS
    eng = _ffi.Engine(str(dev), operands="fp16" if precision == "fp16" else "bf16")
    eng.load_state_dict({k: v.clone() for k, v in sd.items()})
    eng.forward(batch["cur_pluto_feature_torch"], train=True, no_drop=True, bn_update=False, fp32=precision == "fp32")
    out = {}
    for kind in CONTRACT_KINDS:
        stats, flat, _ = eng.loss_backward(kind, _clone_tree(batch))
        grads = {k: torch.zeros_like(sd["planning_decoder.pi_head." + k]).to(dev) for k in PI_KEYS}
        out[kind] = float(eng.loss_finalize(stats, flat, grads).item())
    eng.close()
    return out


def self_launch(args):
    """`python bench.py --gpus N` from a plain shell: run this command under torch.distributed.run in a child process, one rank per GPU of
    this node, and exit with its status."""
    have = torch.cuda.device_count()
    if have < args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} needs {args.gpus} GPUs on this node, torch sees {have}; nothing was measured.\n"
                         f"          (data-parallel correctness without the hardware: tests/test_gpu_dp.py, tests/test_dp_gloo.py)\n")
        sys.exit(2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write("bench.py: launching " + " ".join(cmd) + "\n")
    import subprocess
    sys.exit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--replay", type=int, default=4096, help="total replay scenes (sharded across ranks under weak scaling)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"], help="precision of the headline line")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="roofline counters from the committed profiles/ tables instead of three rocprofv3 --pmc child runs of this command")
    ap.add_argument("--no-precisions", action="store_true", help="skip the fp16 / fp32 companion legs (N = 1)")
    ap.add_argument("--scaling", default="strong", choices=["weak", "strong"],
                    help="which scaling mode is the headline with N > 1 (the other one is reported beside it). strong (default): the reference's "
                         "256-scene minibatch split over the N GPUs (SURVEY.md 8(e)); weak: 256 scenes per GPU per step (global minibatch 256 x N)")
    ap.add_argument("--no-full-update", action="store_true")
    ap.add_argument("--no-tick", action="store_true", help="skip the rollout-tick companion (get_action latency for 1 and 8 CBVs)")
    ap.add_argument("--no-carla", action="store_true", help="skip the CARLA-shaped companion step (49 agents, 60 polygons: the shapes train_cbv really produces)")
    ap.add_argument("--no-e2e", action="store_true", help="skip full_update_e2e (RIFTPluto.train() from a full CBVRolloutBuffer to the reloaded inference model)")
    ap.add_argument("--batch", type=int, default=256, help="scenes per minibatch (diagnostic: 32 = what one of 8 ranks runs under strong scaling)")
    ap.add_argument("--full", action="store_true", help="also measure every companion figure (module docstring); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (loss, probability, pi_head parameters and gradients) as DIR/<name>.npy")
    args = ap.parse_args()
    global BATCH
    BATCH = args.batch
    if not args.full:       # a plain run: the headline leg only
        args.no_cpu_baseline = args.no_roofline = args.no_precisions = args.no_full_update = True
        args.no_tick = args.no_carla = args.no_e2e = True

    if args.gpus > 1 and "RANK" not in os.environ:
        self_launch(args)
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    # (diagnostic, RIFT_BENCH_SAME_GPU=1 under a launcher: every rank on GPU 0 over gloo -- RCCL refuses two ranks on one device -- to walk the
    # N > 1 code of this file and the data-parallel step pipeline on a one-GPU box; the numbers of such a run mean nothing)
    same_gpu = os.environ.get("RIFT_BENCH_SAME_GPU") == "1"
    if same_gpu:
        local_rank = 0
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; start N ranks for --gpus N "
                         f"(or run `python bench.py --gpus N` without a launcher).\n")
        sys.exit(2)
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local_rank:
        sys.stderr.write(f"bench.py: rank {rank} has no GPU (local rank {local_rank}, torch sees {torch.cuda.device_count()} devices).\n")
        sys.exit(2)
    if BATCH % world:
        sys.stderr.write(f"bench.py: strong scaling splits the {BATCH}-scene minibatch over the ranks: {BATCH} % {world} != 0.\n")
        sys.exit(2)

    # stdout carries exactly ONE line (rank 0's JSON): libraries that print banners to fd 1 (RCCL prints its version block at communicator
    # creation) are sent to stderr for the whole run; the saved descriptor is restored for the final print.
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    pg = None
    if world > 1 or os.environ.get("RIFT_BENCH_FORCE_PG") == "1":   # (the env switch exercises the RCCL path on a single GPU)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        if same_gpu:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
        pg = dist.group.WORLD
        if dist.get_world_size() != world:
            sys.stderr.write(f"bench.py: the process group has {dist.get_world_size()} ranks, WORLD_SIZE says {world}.\n")
            sys.exit(2)

    from rift_amd import synthetic as syn
    from rift_amd.planning.fine_tuner.rlft.trainer import RLFTTrainer
    from rift_amd.planning.pluto.model.pluto_model import PlanningModel
    from rift_amd.replay import DeviceReplay

    # ---- the replay: `--replay` scenes seeded per scene index.  weak scaling: rank r holds the contiguous shard [r P, (r + 1) P), P = replay / N,
    # and draws 256 scenes per step from it (global minibatch 256 N); strong scaling: every rank holds the whole replay,
    # all ranks draw the SAME 256-scene minibatch and each takes its contiguous 256 / N slice.  Either way the three exchanges of
    # RLFTTrainer make the step equal the single-process step on the global minibatch.
    t_gen = time.perf_counter()
    per_rank_weak = max(BATCH, args.replay // world)
    ids_weak = range(rank * per_rank_weak, (rank + 1) * per_rank_weak)
    all_ids = range(max(args.replay, per_rank_weak * world)) if world > 1 else ids_weak
    scene_of = {i: syn.make_scene(i) for i in all_ids}
    replays = {"weak": DeviceReplay([scene_of[i] for i in ids_weak], dev, rcap=6)}
    if world > 1:
        replays["strong"] = DeviceReplay([scene_of[i] for i in range(args.replay)], dev, rcap=6)
    scenes = [scene_of[i] for i in ids_weak]
    scenes_cpu = [scene_of[i] for i in sorted(scene_of)][:6 * BATCH]       # the CPU baseline's sample: whole 256-scene minibatches
    t_gen = time.perf_counter() - t_gen

    torch.manual_seed(20250515)   # identical random-init policy on every rank
    model = PlanningModel(radius=120)
    # non-trivial norm/bias/BatchNorm statistics (random-init has all-zero biases)
    sd_cpu = syn.perturbed_state_dict({k: list(v.shape) for k, v in model.state_dict().items()})
    nsteps = args.warmup + args.steps + 8

    def leg(scaling, precision, steps, want_all_outputs=False, want_full_update=False, want_roofline=False, want_steady=False, want_dump=False):
        """Time `steps` update steps in one (scaling, precision) configuration on fresh parameters / optimizer state.
        A generator: the first next() builds the leg (its own model, engine context, trainer, index tensors -- host work, tens of ms), the
        second one runs it and yields the result.  main() builds the headline leg BEFORE it runs the companion legs, so that the headline
        leg's warm-up steps follow the last companion's device work at once: a device left idle while a leg is being built runs the next
        ~30 ms at ramping clocks (per-step times of a leg's first 25 steps fall by 5-10 %, tools/jobs/stepdeltas.py), and W = 5 warm-up
        steps are 4 ms."""
        model = PlanningModel(radius=120)
        strong = scaling == "strong" and world > 1
        replay = replays["strong" if strong else "weak"]
        per_rank = args.replay if strong else per_rank_weak
        local_bs = BATCH // world if strong else BATCH
        global_bs = BATCH if strong else BATCH * world
        model.load_state_dict(sd_cpu)
        model.to(dev)
        model.compute_precision = precision
        model.need_traj = False
        model.train()
        trainer = RLFTTrainer(model, kind="rift", process_group=pg, seed=1)
        eng = trainer.engine
        g = torch.Generator().manual_seed(1000 if strong else 1000 + rank)
        lo = rank * local_bs if strong else 0
        idx = [torch.randperm(per_rank, generator=g)[:BATCH][lo:lo + local_bs].to(torch.int32).to(dev) for _ in range(nsteps)]
        shard = (rank * local_bs, global_bs)

        def step(i):
            fb, b = trainer.gather(replay, idx[i % nsteps])     # (DEFER_SLOTS batch-buffer sets, gathered on the prefetch stream: step k's tail and step k + 1's gather run beside the trunks)
            return trainer.training_step(fb, b, shard=shard)

        def timed(first, count):
            """`count` steps bracketed by barrier + synchronize on both sides; MAX over ranks."""
            trainer.wait_update()          # (data parallel: a tail still held back from the warm-up belongs in front of the timed region)
            if pg is not None:
                torch.distributed.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(first, first + count):
                last = step(i)
            trainer.wait_update()          # (data parallel: the last step's tail is held back until the next forward is issued -- issue it)
            torch.cuda.synchronize()
            if pg is not None:
                torch.distributed.barrier()
            dt = time.perf_counter() - t0
            if pg is not None:
                tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
                torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
                dt = float(tmax.item())
            return dt, last

        yield None
        for i in range(args.warmup):
            step(i)
        dt, loss = timed(args.warmup, steps)
        trainer.wait_update()
        res = {"ms_per_step": dt / steps * 1e3, "value": steps / dt * global_bs, "steps_per_sec": steps / dt, "steps": steps,
               "per_gpu_batch": local_bs, "global_batch": global_bs, "replay_scenes_per_gpu": per_rank, "final_loss": float(loss.item())}
        eng.check_finite()
        if want_dump:
            # what the caller of the last timed step holds behind wait_update(): its loss, the policy logits of its minibatch (this rank's
            # shard) and pi_head after its AdamW update, with the gradients that update used -- copied before any companion runs more steps
            torch.cuda.synchronize()
            res["outputs"] = {"loss": loss.detach().double().cpu().numpy().reshape(-1), "probability": trainer._prob.float().cpu().numpy()}
            for k, p in trainer.params.items():
                res["outputs"]["pi_head." + k] = p.detach().float().cpu().numpy()
                res["outputs"]["pi_head." + k + ".grad"] = p.grad.detach().float().cpu().numpy()

        if (want_all_outputs or want_steady) and steps < 200:
            # companion figure: 200 steps behind the same barriers.  The step pipeline is four steps deep (gather / preparation / history and
            # map encoders of step k + 1 .. k + 3 beside encoder / decoder of step k, head / loss / update of step k behind them): a timed run
            # of K steps pays its fill and drain once (~1 ms), which a 20-step run sees as +0.04 .. 0.05 ms per step
            dt_long, _ = timed(args.warmup, 200)
            trainer.wait_update()
            res["steady_state"] = {"steps": 200, "ms_per_step": dt_long / 200 * 1e3, "value": 200 / dt_long * global_bs,
                                   "note": "the same update steps, 200 of them in one timed region: what an epoch of the update loop runs at"}

        if want_all_outputs:
            # companion figure: the same K steps with EVERY output of PlanningModel.forward computed (trajectory / prediction /
            # ref-free heads -- outputs the RLFT losses never read; the reference's training_step computes them)
            trainer.need_traj = True                 # (the trainer's own output selection: RLFTTrainer.need_traj)
            for i in range(2):
                step(i)
            dt_all, _ = timed(args.warmup, steps)
            trainer.need_traj = False
            res["all_outputs"] = {"ms_per_step": dt_all / steps * 1e3, "value": steps / dt_all * global_bs, "steps_per_sec": steps / dt_all,
                                  "whole_step_mfma_frac": steps / dt_all * global_bs / world * FLOPS_PER_SCENE / (PEAK_BF16_TFLOPS * 1e12),
                                  "note": "trajectory / prediction / ref-free heads computed as the reference's training_step does (1.335 GFLOP per scene)"}

        if want_full_update and world == 1:
            # companion figure: one full policy update as SURVEY.md 8(d) words it -- 16 epochs x (15 training steps + 2 validation steps
            # on the 90 / 10 split of the 4096-scene replay) with the per-epoch host read and scheduler step (single GPU only)
            n_val = per_rank - int(0.9 * per_rank)
            val_idx = [torch.arange(s, min(s + BATCH, n_val), dtype=torch.int32, device=dev) for s in range(0, n_val, BATCH)]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            k = 0
            for epoch in range(16):
                for _ in range(15):
                    step(k)
                    k += 1
                trainer.pop_mean_loss()
                for vi in val_idx:
                    trainer.wait_update()
                    fb, b = replay.collate(eng, vi)
                    trainer.validation_step(fb, b)
                trainer.on_epoch_end()
            torch.cuda.synchronize()
            t_full = time.perf_counter() - t2
            res["full_update"] = {"seconds": t_full, "train_steps": 240, "val_steps": 16 * len(val_idx), "updates_per_sec": 1.0 / t_full,
                                  "note": "16 epochs x (15 x 256-scene training steps + validation of the 10 % split), epoch-end host read included"}

        if want_roofline:
            # roofline leg: per-launch HIP events on the launch stream (separate short pass; every rank runs the profiled steps -- they
            # contain the exchanges -- and rank 0 reports)
            trainer.wait_update()
            piped, trainer.pipeline = trainer.pipeline, False      # per-kernel times of serial launches: the deferred tail would run beside the next trunk
            eng.prof_enable(True)
            nprof = 4
            for i in range(nprof):
                step(args.warmup + steps + i)
            rep = eng.prof_report()
            eng.prof_enable(False)
            trainer.pipeline = piped
            if rank == 0:
                tot_ms = sum(v["ms"] for v in rep.values())
                dom = max(rep.items(), key=lambda kv: kv[1]["ms"])
                gemm_ms = sum(v["ms"] for k, v in rep.items() if k.startswith("gemm_"))
                gemm_fl = sum(v["flops"] for k, v in rep.items() if k.startswith("gemm_"))
                ach = dom[1]["flops"] / (dom[1]["ms"] * 1e-3) / 1e12 if dom[1]["ms"] > 0 else 0.0
                live = collect_counters(dom[0], precision) if (world == 1 and not args.no_pmc) else None
                traffic = live["traffic"] if live else pmc_traffic(dom[0])
                tfile = pmc_traffic_file()
                roof = {"bound": "mfma", "kernel": dom[0], "achieved": ach, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": ach / PEAK_BF16_TFLOPS, "traffic": traffic, "traffic_collected": bool(live),
                        "traffic_source": ("collected in this run: (2*FETCH_SIZE + WRITE_SIZE)*1024 B per launch of this kernel from child runs of this command under "
                                           "rocprofv3 --kernel-trace --pmc (one pass per counter group, 4 profiled steps each; x2 on FETCH_SIZE = the gfx950 "
                                           "correction of MI355X_MICROARCH.md)") if live else
                                          ((os.path.relpath(tfile, REPO) if tfile else "none") +
                                           ": (2*FETCH_SIZE + WRITE_SIZE)*1024 B per launch from separate rocprofv3 --pmc passes of this bench "
                                           "(tools/profile_round.sh); committed measurement, NOT collected in this run (rocprofv3 unavailable or the pass failed)"),
                        "avg_launch_us": dom[1]["ms"] * 1e3 / dom[1]["count"], "launches_per_step": dom[1]["count"] / nprof,
                        "launch_mode": "per-kernel HIP-event times of a SERIAL-launch leg (the profiler puts the forward's chains on one stream and "
                                       "this leg switches the deferred tail off): each kernel alone on the device; the timed region above runs "
                                       "them overlapped (step pipeline), so its step time is below the sum of these",
                        "algorithmic_flops_per_launch": dom[1]["flops"] / dom[1]["count"],
                        "kernel_share_of_gpu_time": dom[1]["ms"] / tot_ms,
                        "all_gemm_tflops": gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0,
                        "gpu_ms_per_step_sum_of_kernels": tot_ms / nprof,
                        "per_kernel_ms_per_step": {k: round(v["ms"] / nprof, 4) for k, v in
                                                   sorted(rep.items(), key=lambda kv: -kv[1]["ms"])[:int(os.environ.get("RIFT_PROF_TOP", "12"))]}}
                if traffic is None:       # loud: a renamed kernel must not turn the traffic figure into a silent null
                    roof["traffic_missing"] = f"no entry for {dom[0]!r} in {os.path.relpath(tfile, REPO) if tfile else 'profiles/ (no table)'}"
                    sys.stderr.write(f"bench.py: WARNING: roofline.traffic is null: {roof['traffic_missing']} -- re-run tools/profile_round.sh\n")
                if live:
                    roof["fetch_kb_per_launch"], roof["write_kb_per_launch"], roof["launches_profiled"] = live["fetch_kb"], live["write_kb"], live["launches_profiled"]
                mf = (live["mfma_flops"], live["mfma_busy_frac"], "collected in this run") if live else pmc_mfma(dom[0])
                if mf is not None and roof["algorithmic_flops_per_launch"]:
                    roof["executed_over_algorithmic_mops"] = mf[0] / roof["algorithmic_flops_per_launch"]
                    roof["mfma_busy_frac"] = mf[1]
                    roof["mfma_counters_source"] = mf[2] + ": SQ_INSTS_VALU_MFMA_MOPS_BF16 x 512 FLOP and SQ_VALU_MFMA_BUSY_CYCLES / (4 SQ_BUSY_CU_CYCLES) per launch (committed pass)"
                res["roofline"] = roof
        trainer.close()
        model.release_engine()       # (the context's side stream goes with it: a later leg's streams must not end up sharing hardware queues)
        yield res

    def full_update_e2e():
        """What the user of `scripts/run.py --mode train_cbv` waits for between two rollout phases: RIFTPluto.train(e_i) from a FULL
        CBVRolloutBuffer (4096 transitions committed through store(), which lays each one into the pinned host arena as the rollout
        produces it) to the reloaded inference model -- checkpoint load, trainer, arena upload, 16 epochs x (15 training + 2 validation
        steps), top-1 checkpoint on disk, inference-model reload + re-bind, buffer reset.  Two updates: the first also builds the
        training model and its context."""
        import shutil
        import tempfile
        from rift_amd.gym_carla.buffer.cbv_rollout_buffer import CBVRolloutBuffer
        from rift_amd.planning import CBV_POLICY_LIST
        from rift_amd.planning.pluto.feature_builder.pluto_feature import PlutoFeature
        root = tempfile.mkdtemp(prefix="rift_e2e_")
        try:
            pol = CBV_POLICY_LIST['rift_pluto']({'num_scenario': 1, 'ROOT_DIR': root, 'model_path': 'ckpt', 'device': str(dev),
                                                 'compute_precision': args.precision}, None)
            pol.pluto_model.load_state_dict(sd_cpu)
            pol.load_model(resume=True)
            pol.set_mode('train')
            keys = ['CBVs_obs', 'CBVs_reward', 'CBVs_done', 'CBVs_actions_old_group_logits', 'CBVs_group_advantage']
            buf = CBVRolloutBuffer(1, 'train_cbv', {'buffer_capacity': args.replay, 'data_keys': keys, 'obs': {'max_agent': 63},
                                                    'host_caps': {'Mp': 20, 'R': 6}})
            pol.set_buffer(buf)
            res = {}
            for upd in range(2):
                t_store, i = 0.0, 0
                while not buf.buffer_full:                      # 8-step episodes of one CBV, as the rollout would commit them
                    for k in range(8):
                        s = scenes[i % len(scenes)]
                        ex = s["extras"]
                        d = {'CBV_ids': [[3]], 'CBVs_obs': [{3: {'raw_pluto_feature': PlutoFeature(data=s["feature"])}}],
                             'CBVs_reward': [{3: 0.0}], 'CBVs_done': [{3: k == 7}],
                             'CBVs_actions_old_group_logits': [{3: {'logits': ex["old_group_logits"].numpy(), 'valid_mask': ex["old_group_logits_mask"].numpy()}}],
                             'CBVs_group_advantage': [{3: {'advantage': ex["group_advantage"].numpy(), 'valid_mask': ex["group_advantage_mask"].numpy()}}]}
                        t0 = time.perf_counter()
                        buf.store(d)
                        t_store += time.perf_counter() - t0
                        i += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit = pol.train(upd)
                pol.pluto_model.engine()                        # the reloaded inference model bound to its context: ready for the next tick
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res["first_update" if upd == 0 else "steady"] = {
                    "seconds": dt, "store_us_per_transition": t_store / max(i, 1) * 1e6,
                    "host_timeline_s": {k: round(v, 4) for k, v in fit["timing"].items()}, "best_val_loss": fit["best_val_loss"]}
            out = dict(res["steady"])
            out["first_update"] = res["first_update"]
            pol.pluto_model.release_engine()
            if pol.train_model is not None:
                pol.train_model.release_engine()
            out["note"] = ("RIFTPluto.train(e_i) on a full 4096-transition CBVRolloutBuffer -> reloaded inference model: checkpoint load, arena upload from the pinned host "
                           "mirror filled at store() time, 16 epochs x (15 training + 2 validation steps), top-1 checkpoint on disk, reload, buffer reset; "
                           "`seconds` = the second update of the process (the first also builds the training model and its context); store() cost is paid during the rollout")
            return out
        finally:
            shutil.rmtree(root, ignore_errors=True)

    head_scaling = args.scaling if world > 1 else "weak"      # (one GPU: the two coincide -- 256 scenes per step on the one rank)
    # the companion legs run first, the headline leg last, every leg built before the first one runs (see leg())
    def built(*a, **kw):
        g = leg(*a, **kw)
        next(g)
        return g

    head_leg = built(head_scaling, args.precision, args.steps, want_all_outputs=args.full, want_full_update=not args.no_full_update,
                     want_roofline=not args.no_roofline, want_dump=args.dump_outputs is not None)
    other = None
    if world > 1 and args.full:
        other_scaling = "strong" if head_scaling == "weak" else "weak"
        other = (other_scaling, next(built(other_scaling, args.precision, args.steps)))
    precisions = None
    keep = ("ms_per_step", "value", "steps_per_sec", "steps", "final_loss")
    if world == 1 and not args.no_precisions:
        precisions = {}
        # (the 16-bit companion also runs its 200-step region: at the driver's K = 20 a leg sits on the device's clock ramp -- profiles/NOTES_r06.md --
        # and the order of the legs decides who pays how much of it; the steady states are what compares the two 16-bit builds)
        todo = [(p, built("weak", p, args.steps if p != "fp32" else max(5, min(args.steps, 20)), want_steady=p != "fp32"))      # (the layer-by-layer fp32 step is several times longer)
                for p in ("fp32", "fp16", "bf16") if p != args.precision]
        for p, g in todo:
            r = next(g)
            precisions[p] = {k: r[k] for k in keep}
            if "steady_state" in r:
                precisions[p]["steady_ms_per_step"] = r["steady_state"]["ms_per_step"]
    if precisions is None and other is None:
        # without companion legs in front, the headline's warm-up would start on an idle device, whose clocks put its K = 20 region ~6 %
        # above the same steps behind the companions (profiles/NOTES_r06.md): a throwaway leg of 200 update steps takes their place (its own
        # model and trainer -- the headline's steps, and what they compute, are the same as behind the companions)
        next(built(head_scaling, args.precision, 200))
    head = next(head_leg)
    if args.dump_outputs is not None and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        outs = head.pop("outputs")
        if sum(a.nbytes for a in outs.values()) > 64 << 20:      # (a large --batch: a fixed, seeded sample of the minibatch's rows)
            rows = torch.randperm(outs["probability"].shape[0], generator=torch.Generator().manual_seed(0))[:4096].sort().values.numpy()
            outs["probability"] = outs["probability"][rows]
        for name, a in outs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    contract = None
    if world == 1 and rank == 0 and not args.no_cpu_baseline and BATCH == 256:
        # north_star's precision contract, machine-readable: the four objectives of the parity test's 256-scene batch per compute precision
        # (device side here -- BEHIND the headline leg: three short-lived contexts in front of it leave the device idle for tenths of a second
        # and the headline's 20 steps then run at ramping clocks, measured +0.05 ms per step; the oracle side runs with the CPU baseline below
        # and the errors are filled in there)
        cb = contract_batch()
        contract = {"batch": cb, "device": {p: contract_device_losses(dev, sd_cpu, cb, p) for p in ("bf16", "fp16", "fp32")}}
    # the companions that build policies / contexts of their own run BEHIND the headline leg: every further live context adds streams that
    # share hardware queues with the headline trainer's (measured: headline 0.66 -> 0.75 ms per step with the end-to-end update ahead of it)
    e2e = full_update_e2e() if (world == 1 and rank == 0 and not args.no_e2e and not args.no_full_update and BATCH == 256) else None
    carla = None
    if world == 1 and rank == 0 and not args.no_carla and BATCH == 256:
        # companion figure: the update step at the shapes `scripts/run.py --mode train_cbv` really produces (rift_pluto.yaml:35-36: max_agent 48 ->
        # <= 49 agents with the CBV, ~60 polygons inside radius 120, R ~ U{1..6}): N = 109 token slots > 96, i.e. the
        # dense-traffic variants of the scene encoder and decoder (enc_w_kernel, dec_w_kernel<., true>) instead of the 96-token kernels
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import shape_step
        carla = {}
        for shp in ("carla", "carla-ragged"):
            r = shape_step.run(shp, bs=BATCH, precision=args.precision, steps=60, verbose=False)
            carla[shp] = {k: r[k] for k in ("A", "Mp", "tokens", "ms_per_step", "scenes_per_s", "us_per_scene", "per_kernel_ms")}
    tick = None
    if world == 1 and rank == 0 and not args.no_tick and BATCH == 256:
        # companion figure of the rollout side: what the simulator loop waits for every tick
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import tick_latency
        tick = tick_latency.run(ticks=30, cbvs=(1, 8))
        tick["note"] = ("host wall time of one `get_action` for K CBVs of one environment at the CARLA shapes (fp16 operands, the policies' default): "
                        "'pluto/eval' = eval forward with every output -> candidate trimming -> PID; 'rift_pluto/train' = that + the device-side "
                        "group advantage of every CBV (rollout, neighbour forecast, collision / off-road flags, return, z-score); tools/tick_latency.py")
    if precisions is not None:
        precisions[args.precision] = {k: head[k] for k in keep}
        if "steady_state" in head:
            precisions[args.precision]["steady_ms_per_step"] = head["steady_state"]["ms_per_step"]
        precisions["note"] = ("the same update steps per compute precision: bf16 / fp16 = the fused kernels on bf16 / fp16 MFMA operands; fp32 = exact "
                              "v_mfma_f32_16x16x4_f32 layer by layer (the reference's `precision: 32`).  Parity per mode: tests/test_gpu_parity.py header")

    if rank == 0:
        strong = head_scaling == "strong" and world > 1
        line = {
            "metric": f"policy-update scenes/sec ({BATCH}-scene RIFT update steps on a 4096-scene replay)",
            "value": head["value"], "unit": "scenes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": ("strong" if strong else "weak") if world > 1 else None, "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic",
            "steps_per_sec": head["steps_per_sec"],
            "rccl_ranks": torch.distributed.get_world_size() if pg is not None else 0,          # ranks of the process group the exchanges ran over
            "collective_backend": (torch.distributed.get_backend() if pg is not None else None),
            "config": {"workload": "BASELINE configs[2]/[3]: full rift_pluto CBV policy, 4096-scene synthetic replay "
                                   "(64 agents x 21 steps, 20 polygons x 3 x 20 pts, R~U{1..6} x 120 ref pts, 12 modes), "
                                   "RIFT loss, pi_head trainable",
                       "per_gpu_batch": head["per_gpu_batch"], "global_batch": head["global_batch"], "replay_scenes_per_gpu": head["replay_scenes_per_gpu"],
                       "parallelism": f"dp{world}", "train_mode": "dropout+droppath+state-dropout, BN batch stats"
                                                                + (" over the global minibatch (3 all-reduces per step)" if world > 1 else ""),
                       "outputs": "probability (the trajectory / prediction / ref-free heads feed no RLFT loss and are skipped; "
                                  "all_outputs = the same steps with every output of PlanningModel.forward computed)"},
            # whole-step fraction of the dense bf16 MFMA peak, priced at the algorithmic FLOPs of what each variant executes
            "whole_step_mfma_frac": head["value"] / world * FLOPS_PER_SCENE_LOSS / (PEAK_BF16_TFLOPS * 1e12),
            **({"all_outputs": head["all_outputs"]} if "all_outputs" in head else {}),
            **({"steady_state": head["steady_state"]} if "steady_state" in head else {}),
            "final_loss": head["final_loss"], "replay_gen_s": round(t_gen, 2), "replay_hbm_mb": round(replays["weak"].nbytes() / 1e6, 1),
        }
        if world > 1:
            notes = {"strong": "SURVEY.md 8(e): the reference's 256-scene minibatch split contiguously over the ranks (15 optimizer steps per epoch of the 4096-scene replay, as the reference); steps/s is the reference's optimizer-step rate",
                     "weak": "256 scenes per GPU per step: the reference's update with train_batch_size = 256 N (fewer, larger optimizer steps per epoch)"}
            for name, r in [(head_scaling, head)] + ([other] if other is not None else []):
                line[name] = {k: r[k] for k in ("ms_per_step", "value", "steps_per_sec", "per_gpu_batch", "global_batch", "replay_scenes_per_gpu")}
                line[name]["note"] = notes[name]
        if "full_update" in head:
            line["full_update"] = head["full_update"]
        if e2e is not None:
            line["full_update_e2e"] = e2e
        if carla is not None:
            for shp in carla:
                carla[shp]["step_time_vs_benchmark_shape"] = carla[shp]["ms_per_step"] / (head.get("steady_state", head)["ms_per_step"])
            carla["note"] = ("the same 256-scene update step at the shapes train_cbv produces (49 agent slots, 60 polygon slots, 109 token slots; 'carla-ragged': "
                             "per-scene agent / polygon counts drawn below those caps, as a rollout yields them); token ratio to the benchmark shape 109 / 84 = 1.30")
            line["carla_shape"] = carla
        if tick is not None:
            line["rollout_tick"] = tick
        if precisions is not None:
            line["precisions"] = precisions
        if "roofline" in head:
            line["roofline"] = head["roofline"]
        # the companions the review reads, as flat scalars inside `config` (the driver's record keeps `config` and `roofline` whole and drops
        # other top-level keys): the reference-equivalent step (every output of PlanningModel.forward: pluto_model.py:173-199) and the
        # steady state (200 steps in one region)
        if "all_outputs" in head:
            line["config"]["all_outputs_ms_per_step"] = head["all_outputs"]["ms_per_step"]
            line["config"]["all_outputs_value"] = head["all_outputs"]["value"]
        if "steady_state" in head:
            line["config"]["steady_state_ms_per_step"] = head["steady_state"]["ms_per_step"]
            line["config"]["steady_state_value"] = head["steady_state"]["value"]
        if not args.no_cpu_baseline:
            # (rank 0's host cores; the other ranks wait at the closing barrier.  A 256-scene CPU step whatever N is: the reference is single-device)
            line["cpu_baseline"] = cpu_baseline(scenes_cpu, sd_cpu, contract["batch"] if contract is not None else None)
            want = line["cpu_baseline"].pop("contract_oracle")
            if contract is not None:
                pc = {"tolerance": 1e-4, "batch": "256 scenes (synthetic ids 1000..1255), train-mode BatchNorm batch statistics, drops disabled; "
                                                  "the batch of tests/test_gpu_parity.py::test_benchmark_batch_objectives_in_16bit_modes",
                      "checker": "oracle/ (PyTorch-CPU fp32 restatement of the reference, pinned to reference-generated goldens); computed in this run",
                      "oracle_loss": want}
                for prec, got in contract["device"].items():
                    errs = {k: abs(got[k] - want[k]) for k in CONTRACT_KINDS}
                    entry = {"loss_err_vs_oracle": errs, "max_loss_err_vs_oracle": max(errs.values()), "meets_north_star_1e-4": bool(max(errs.values()) < 1e-4),
                             "objectives_inside_1e-4": [k for k in CONTRACT_KINDS if errs[k] < 1e-4]}
                    pc[prec] = entry
                    if precisions is not None and prec in precisions:
                        precisions[prec].update({"max_loss_err_vs_oracle": entry["max_loss_err_vs_oracle"], "loss_err_vs_oracle": errs,
                                                 "meets_north_star_1e-4": entry["meets_north_star_1e-4"]})
                line["precision_contract"] = pc
                line["headline_meets_north_star_1e-4"] = pc[args.precision]["meets_north_star_1e-4"]
                # the fastest 16-bit mode whose four objectives all sit inside north_star's 1e-4 on this batch, with its own step time
                clean = [(precisions[q]["ms_per_step"], q) for q in ("bf16", "fp16") if precisions is not None and q in precisions and pc.get(q, {}).get("meets_north_star_1e-4")]
                if clean:
                    ms, q = min(clean)
                    line["config"]["contract_clean_dtype"] = q
                    line["config"]["contract_clean_ms_per_step"] = ms
                    line["config"]["contract_clean_value"] = precisions[q]["value"]
                    line["config"]["contract_clean_max_loss_err"] = pc[q]["max_loss_err_vs_oracle"]
                    if "steady_ms_per_step" in precisions[q]:      # (200 steps in one region: compare with config.steady_state_ms_per_step)
                        line["config"]["contract_clean_steady_ms_per_step"] = precisions[q]["steady_ms_per_step"]
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)
    if pg is not None:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
