"""Same launches, same bits: an A/B of two builds of the library over the paths of the unroll's forward.

For every configuration below and every library, a fresh child process (``AAA_LIB`` names the library) runs one
forward and one backward with the kernel timers on, twice, and prints per run: every timer class's (launches,
work, variant), the sha256 of each deterministic output's bytes (logits, values, attention maps, hT, cT, dh0, dc0
and the stateful core's hT / cT / dcore_h0 / dcore_c0) and of every region aaa_workspace_region grants, read after
the forward from a workspace zeroed before it.  The 34 gradients are atomic sums whose order differs from process
to process, so they are compared by the norm-relative difference over the whole flat gradient.

    python tools/ab_forward_launches.py --parent <parent's libaaa.so> --lib <this tree's libaaa.so> --out <dir>

runs two processes on the parent's library and one on this tree's, and requires
  * equal timer triples, output digests and region digests in all six runs of a configuration, and
  * this tree's gradient difference against a parent process to be at most twice the difference between the two
    parent processes (the larger of the two runs on either side).
It writes <dir>/launch_ab.json and exits non-zero where a requirement fails.  A child that fails ends the run: no
further process is started on the device.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 3
MASK = [(0, 1), (2, 0)]   # episode starts (t, b)
# name -> (dtype, B, H, W, nq, stateful core, uint8 frames, mask, environment)
CONFIGS = {
    "fp32_B2": ("fp32", 2, 64, 64, 4, False, False, False, {}),
    "fp32_B2_batched_xpart": ("fp32", 2, 64, 64, 4, False, False, False, {"AAA_FUSED_X": "0"}),
    "fp32_B2_stateful_mask": ("fp32", 2, 64, 64, 4, True, False, True, {}),
    "bf16_B2": ("bf16", 2, 64, 64, 4, False, False, False, {}),
    "bf16_B32_u8_paired_frames": ("bf16", 32, 84, 84, 4, False, True, False, {}),
    "fp32_B32_u8_frame_group": ("fp32", 32, 84, 84, 4, False, True, False, {}),
    "fp32_B32_u8_frame_group_mask": ("fp32", 32, 84, 84, 4, False, True, True, {}),
    "bf16_B5_168_band": ("bf16", 5, 168, 168, 8, False, False, False, {}),   # tests/test_gpu_band.py's shape
}
CHILD_TIMEOUT = 240   # seconds: a child is a few seconds of work after the imports


def child(name: str, grad_path: str) -> None:
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import attention
    from aaa_amd import _native as N
    from aaa_amd import detinit
    from aaa_amd.runtime import UnrollRunner

    dtype, B, H, W, nq, stateful, u8, masked, _ = CONFIGS[name]
    dev = torch.device("cuda:0")
    r = UnrollRunner(B, T, H, W, nq, 18, dtype, dev, stateful_core=stateful, frames_u8=u8)
    params = detinit.deterministic_params(0, 18, nq)
    flat = torch.cat([torch.from_numpy(np.asarray(v, np.float32)).reshape(-1) for v in params.values()]).to(dev)
    packed, ws = r.new_packed(), r.new_workspace()
    r.pack(flat, packed)
    basis = attention.SpatialBasis(r.h, r.w).S.to(dev).contiguous()
    fr = detinit.frames_u8(1234, (T, B, H, W, 3))
    frames = torch.from_numpy(fr if u8 else fr.astype(np.float32)).to(dev)

    def cot(seed, shape, scale=1.0):
        return (torch.from_numpy(detinit.cotangent(seed, shape)) * scale).to(dev)

    h0, c0 = cot(11, r.state_shape(), 0.5), cot(12, r.state_shape(), 0.5)
    dl, dv, dhT, dcT = cot(2, (T, B, 18)), cot(3, (T, B, 18)), cot(13, r.state_shape()), cot(14, r.state_shape())
    core = (cot(15, (B, 256), 0.5), cot(16, (B, 256), 0.5)) if stateful else None
    dcore = (cot(17, (B, 256)), cot(18, (B, 256))) if stateful else None
    reset = None
    if masked:
        reset = torch.zeros(T, B, device=dev)
        for t, b in MASK:
            reset[t, b] = 1.0

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    runs = []
    for k in range(2):
        ws.zero_()
        N.pair_status(clear=True)
        N.timing_enable(True)
        try:
            fwd = r.forward(flat, packed, basis, frames, ws, h0=h0, c0=c0, want_state=True, core=core, reset=reset)
            torch.cuda.synchronize()
            regions = {}
            for region in range(64):
                off, nb = N.ctypes.c_size_t(), N.ctypes.c_size_t()
                if r.lib.aaa_workspace_region(N.ctypes.byref(r.cfg), region, N.ctypes.byref(off), N.ctypes.byref(nb)) == 0:
                    regions[str(region)] = sha(ws[off.value:off.value + nb.value])
            bwd = r.backward(flat, packed, basis, frames, ws, dl, dv, dhT, dcT, want_state_grads=True, dcore=dcore,
                             want_core_grads=stateful, reset=reset)
            torch.cuda.synchronize()
            timers = {}
            for kind in range(N.TIMER_N):
                s = N.timing_stats(kind)
                timers[str(kind)] = [s["launches"], s["work"], s["variant"]]
        finally:
            N.timing_enable(False)
        stranded = N.pair_status(clear=True)
        names = ["logits", "values", "attn", "hT", "cT"] + (["core_hT", "core_cT"] if stateful else [])
        exact = {n: sha(t) for n, t in zip(names, fwd)}
        names = ["dh0", "dc0"] + (["dcore_h0", "dcore_c0"] if stateful else [])
        exact.update({n: sha(t) for n, t in zip(names, bwd[1:])})
        np.save(f"{grad_path}.{k}.npy", bwd[0].cpu().numpy())
        runs.append({"timers": timers, "exact": exact, "regions": regions, "stranded": stranded})
    print(json.dumps({"config": name, "lib": N.LIB_PATH, "runs": runs}), flush=True)


def norm_rel(a, b):
    import numpy as np
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--grads")
    ap.add_argument("--parent")
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.grads)
        return 0
    import numpy as np
    os.makedirs(a.out, exist_ok=True)
    report, ok = {}, True
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.configs.split(","):
            procs = {}
            for who, lib in (("parentA", a.parent), ("parentB", a.parent), ("change", a.lib)):
                env = dict(os.environ, AAA_LIB=os.path.abspath(lib), **CONFIGS[name][-1])
                gp = os.path.join(tmp, f"{name}.{who}")
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--grads", gp], env=env,
                                   capture_output=True, text=True, timeout=CHILD_TIMEOUT)
                if p.returncode != 0:
                    print(f"{name}/{who}: child exited {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}",
                          flush=True)
                    return 2
                procs[who] = (json.loads(p.stdout.strip().splitlines()[-1]),
                              [np.load(f"{gp}.{k}.npy") for k in range(2)])
            runs = [r for who in procs for r in procs[who][0]["runs"]]
            first = runs[0]
            g = {who: procs[who][1] for who in procs}
            pvp = [norm_rel(g["parentB"][k], g["parentA"][k]) for k in range(2)]
            cvp = [norm_rel(g["change"][k], g["parentA"][k]) for k in range(2)]
            row = {
                "timers_equal": all(r["timers"] == first["timers"] for r in runs),
                "exact_outputs_equal": all(r["exact"] == first["exact"] for r in runs),
                "regions_equal": all(r["regions"] == first["regions"] for r in runs),
                "stranded": sum(r["stranded"] for r in runs),
                "exact_outputs": sorted(first["exact"]),
                "regions": sorted(first["regions"], key=int),
                "grads_parent_vs_parent_norm_rel": pvp,
                "grads_change_vs_parent_norm_rel": cvp,
                "grads_change_vs_other_parent_norm_rel": [norm_rel(g["change"][k], g["parentB"][k]) for k in range(2)],
                "grads_within_bound": max(cvp) <= 2.0 * max(pvp),
                "timers": first["timers"],
            }
            row["ok"] = bool(row["timers_equal"] and row["exact_outputs_equal"] and row["regions_equal"]
                             and row["grads_within_bound"] and row["stranded"] == 0)
            if not row["timers_equal"]:
                row["timers_by_process"] = {who: [r["timers"] for r in procs[who][0]["runs"]] for who in procs}
            ok &= row["ok"]
            report[name] = row
            print(f"{name}: timers {'equal' if row['timers_equal'] else 'DIFFER'}, outputs "
                  f"{'equal' if row['exact_outputs_equal'] else 'DIFFER'}, {len(row['regions'])} regions "
                  f"{'equal' if row['regions_equal'] else 'DIFFER'}, grads parent-vs-parent {max(pvp):.2e} "
                  f"change-vs-parent {max(cvp):.2e} ({'within' if row['grads_within_bound'] else 'OUTSIDE'} 2x)", flush=True)
            with open(os.path.join(a.out, "launch_ab.json"), "w") as f:
                json.dump(report, f, indent=1)
    print("PASS" if ok else "FAIL", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
