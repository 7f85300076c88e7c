"""KernelPlan::nat_group (csrc/fwd_kernels.h) over its inputs, compiled with the system compiler like tests/test_host_api.py does: the
DropPath grouping of NAT levels 1 and 2 is on exactly in a train-mode forward with drops on the compacted wave-private history chain,
and RIFT_NAT_GROUP=0 / RIFT_NO_SKIP=1 switch it off."""
import itertools
import os
import shutil
import subprocess

import pytest


def test_nat_group_plan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    default = dict(nat_fused=1, dec_fused=1, enc_fused=1, pe_fused=1, fo_fused=1, fpn_fused=1, ego_fused=1, heads_fused=1, pi_fused=1, fo_w=1, pe_w=1,
                   nat_compact=1, pe_live=1, pe_pack=1, rank_in_prep=1, enc112=1, dec_defer_max=-1, dec_split=1, dec_layers=4, dec_ts=0,
                   fp32=0, train=0, drop=0, need_traj=0, want_traj=0, defer_head=0, prof_on=0, forked=1, bs=32, A=64, Mp=20, S=0, R=4, enc_nw=8)
    flags = ["nat_fused", "fpn_fused", "nat_compact", "fp32", "drop", "nat_group", "no_skip"]
    code = ['#include <cstdio>', '#include "fwd_kernels.h"', 'int main() {', '  KernelIn in;'] + [f'  in.{k} = {v};' for k, v in default.items()]
    code += ['  { const KernelPlan p = plan_kernels(in); printf("%d\\n", (int)p.nat_group); in.drop = true; in.train = true; printf("%d\\n", (int)plan_kernels(in).nat_group); }']
    for k in flags:
        code.append(f'  for (int {k} = 0; {k} < 2; ++{k}) {{ in.{k} = {k} != 0;')
    code.append('    printf("%d\\n", (int)plan_kernels(in).nat_group);' + ' }' * len(flags))
    code += ['  return 0;', '}']
    src = tmp_path / "gplan.cpp"
    src.write_text("\n".join(code))
    exe = tmp_path / "gplan"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-I", os.path.join(repo, "rift_amd", "csrc"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [0, 1], "the switches' defaults: off in an eval forward, on in a train forward with drops"
    rows = list(itertools.product((0, 1), repeat=len(flags)))
    assert len(got) == 2 + len(rows)
    for v, g in zip(rows, got[2:]):
        i = dict(zip(flags, v))
        want = i["nat_fused"] and not i["fp32"] and i["fpn_fused"] and i["nat_compact"] and i["drop"] and i["nat_group"] and not i["no_skip"]
        assert g == int(bool(want)), i
