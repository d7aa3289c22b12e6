"""Timing and kernel resources of the factor imputation (``csrc/k_ximpute.hip``): writes
``ximpute_timing.txt`` and ``ximpute_resources.txt`` into ``--out_dir``.

    python tools/impute_profile.py [--out_dir profiles] [--repeats 9] [--factors 6]

GPU only. Two panels with a planted factor structure (log-normal levels, 2 % of the entries NaN, a
tenth of the rows dead; seeded, generated on the device) are ranked in place by ``k_xrank`` with a
NaN fill: the three bench splits 240 / 60 / 300 x 3000 x 46 and one 16-period chunk of 30000 x 512
(0.98 GB). Per piece, device events around the call, median / min of the warm repeats:
  k_ximp_gram   ``_dlap_hip.characteristic_moments`` into buffers allocated before the window;
  k_ximp_fill   ``_dlap_hip.xs_fill`` out of place, with the loadings of the kernel's own moments;
  torch         a route that lives here only, on the same GPU: the moments as two masked fp32
                ``bmm`` (z' z and o' o), the fill as ``O @ P`` and ``Z @ lam`` by ``bmm``, a batched
                ``torch.linalg.solve`` and a ``where``;
  eigh          ``xs_loadings`` (host numpy float64) for the piece's periods, a host clock.
The tool also reports the largest difference between the kernels and the torch route. Resources:
``hipcc -Rpass-analysis=kernel-resource-usage`` of the kernel file."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearninginassetpricing_paperreplication_amd.data import transforms as tr  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.dataset import MISSING_VALUE  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.ops import native  # noqa: E402

# label: (N, F, periods of each timed piece)
PANELS = {"bench": (3000, 46, (240, 60, 300)), "scaled": (30000, 512, (16,))}
GAMMA = 0.01


def ranked_panel(nat, T, N, F, seed, Kt=4):
    g = torch.Generator(device="cuda").manual_seed(seed)
    fac = torch.randn((T, N, Kt), generator=g, device="cuda")
    B = torch.randn((T, Kt, F), generator=g, device="cuda")
    x = torch.bmm(fac, B).mul_(0.8 / Kt ** 0.5)
    x.add_(torch.randn((T, N, F), generator=g, device="cuda"), alpha=0.6).exp_()
    x[torch.rand((T, N, F), generator=g, device="cuda") < 0.02] = float("nan")
    ok = (torch.rand((T, N), generator=g, device="cuda") > 0.1).to(torch.uint8)
    cnt = torch.empty((T, F), dtype=torch.int32, device="cuda")
    nat.rank_characteristics(x.data_ptr(), ok.data_ptr(), x.data_ptr(), cnt.data_ptr(), T, N, F, float(tr.THR),
                             float("nan"), MISSING_VALUE, torch.cuda.current_stream().cuda_stream)
    return x, ok


def _events(fn, repeats):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(repeats + 1):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
        del out
    return statistics.median(ms[1:]), min(ms[1:])


def torch_moments(y, ok):
    o = ok.bool()[:, :, None] & (y == y)
    z = torch.where(o, y, torch.zeros_like(y))
    of = o.to(torch.float32)
    return torch.bmm(z.transpose(1, 2), z), torch.bmm(of.transpose(1, 2), of)


def torch_fill(y, ok, lam, gamma):
    T, N, F = y.shape
    K = lam.shape[2]
    o = ok.bool()[:, :, None] & (y == y)
    z = torch.where(o, y, torch.zeros_like(y))
    P = (lam[:, :, :, None] * lam[:, :, None, :]).reshape(T, F, K * K)
    A = torch.bmm(o.to(torch.float32), P).reshape(T, N, K, K) + gamma * torch.eye(K, device=y.device)
    g = torch.linalg.solve(A, torch.bmm(z, lam)[:, :, :, None])[:, :, :, 0]
    fit = torch.bmm(g, lam.transpose(1, 2)).clamp_(-0.5, 0.5)
    return torch.where(ok.bool()[:, :, None] & ~o, fit, y)


def time_panel(label, repeats, K):
    nat = native.load(required=True)
    N, F, pieces = PANELS[label]
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for i, T in enumerate(pieces):
        y, ok = ranked_panel(nat, T, N, F, seed=200 + i)
        S = torch.empty((T, F, F), dtype=torch.float64, device="cuda")
        C = torch.empty((T, F, F), dtype=torch.int32, device="cuda")
        res = torch.empty_like(y)
        gmd, gmn = _events(lambda: nat.characteristic_moments(y.data_ptr(), ok.data_ptr(), S.data_ptr(), C.data_ptr(),
                                                              T, N, F, stream), repeats)
        t0 = time.perf_counter()
        lam_h, explained = tr.xs_loadings(S.cpu().numpy(), C.cpu().numpy(), K)
        eigh_s = time.perf_counter() - t0
        lam = torch.from_numpy(lam_h).cuda()
        fmd, fmn = _events(lambda: nat.xs_fill(y.data_ptr(), ok.data_ptr(), lam.data_ptr(), res.data_ptr(), T, N, F,
                                               lam.shape[2], GAMMA, stream), repeats)
        tgmd, tgmn = _events(lambda: torch_moments(y, ok), min(repeats, 3))
        tfmd, tfmn = _events(lambda: torch_fill(y, ok, lam, GAMMA), min(repeats, 3))
        tS, tC = torch_moments(y, ok)
        dS = float(((tS.double() - S).abs().max() / S.abs().max()).item())
        sameC = bool(torch.equal(tC.to(torch.int32), C))
        del tS, tC
        tf = torch_fill(y, ok, lam, GAMMA)
        hole = ok.bool()[:, :, None] & (y != y)
        dF = float((tf - res)[hole].abs().max().item())
        holes = int(hole.sum().item())
        del tf, hole
        flop = 2.0 * T * N * F * F
        out.append(f"  {label:<6s} {T:3d} x {N} x {F} ({y.numel() * 4 / 1e6:7.1f} MB, {holes} holes, K {lam.shape[2]}, explained "
                   f"{float(explained.mean()):.3f})  k_ximp_gram gpu_ms {gmd:9.3f} / {gmn:9.3f} ({flop / gmd / 1e9:7.2f} TFLOP/s of 2 T N F^2)  "
                   f"torch bmm ms {tgmd:9.3f} / {tgmn:9.3f}  torch / kernel {tgmd / gmd:6.2f}   "
                   f"k_ximp_fill gpu_ms {fmd:9.3f} / {fmn:9.3f} ({2 * y.numel() * 4 / fmd / 1e6:7.1f} GB/s of y read + out written)  "
                   f"torch solve route ms {tfmd:9.3f} / {tfmn:9.3f}  torch / kernel {tfmd / fmd:6.2f}   "
                   f"host eigh {eigh_s:7.3f} s   max |S - S_torch| / max |S| {dS:.2e}, C {'same' if sameC else 'DIFFER'}, "
                   f"max |fill - fill_torch| {dF:.2e}")
        del y, ok, S, C, res, lam
        torch.cuda.empty_cache()
    return out


def resources():
    """VGPRs, AGPRs, scratch, spills, occupancy of the two kernels from the compiler's remarks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "csrc", "k_ximpute.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{os.path.join(ROOT, 'csrc')}",
                            "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                            os.path.join(d, "k.o")], capture_output=True, text=True)
    if r.returncode != 0:
        return [f"  (hipcc failed: {r.stderr[-200:]})"]
    rows, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: +(?:Function Name: (\S+)|([A-Za-z ]+?)(?: \[[^\]]*\])?: +(\d+))", ln)
        if not m:
            continue
        if m.group(1):
            cur = {"name": m.group(1)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    out = ["  kernel           SGPRs  VGPRs  AGPRs  scratch B/lane  VGPR spills  SGPR spills  waves/SIMD  static LDS B"]
    for c in rows:
        k = re.search(r"(k_ximp_fill|k_ximp_gram)ILi(\d+)E", c["name"])
        name = f"{k.group(1)}<{k.group(2)}>" if k else c["name"]
        out.append(f"  {name:<15s} {c.get('TotalSGPRs', -1):6d} {c.get('VGPRs', -1):6d} {c.get('AGPRs', -1):6d}  "
                   f"{c.get('ScratchSize', -1):14d}  {c.get('VGPRs Spill', -1):11d}  {c.get('SGPRs Spill', -1):11d}  "
                   f"{c.get('Occupancy', -1):10d}  {c.get('LDS Size', -1):12d}")
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out_dir", default=os.path.join(ROOT, "profiles"))
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--factors", type=int, default=6)
    p.add_argument("--resources_only", action="store_true", help="no GPU: write the resources file only")
    a = p.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    rl = ["Kernel resources of k_ximp_gram and k_ximp_fill<K> (gfx950, -O3; hipcc -Rpass-analysis=kernel-resource-usage).",
          "N, F and T are run-time arguments; the LDS is dynamic: k_ximp_gram 51712 B, k_ximp_fill "
          "(ceil(F / 32) 32 (NC + 2) + 256 (NC + 1)) 4 B with NC = 16 ceil((K + K (K + 1) / 2) / 16).", ""] + resources()
    with open(os.path.join(a.out_dir, "ximpute_resources.txt"), "w") as f:
        f.write("\n".join(rl) + "\n")
    print("\n".join(rl))
    if a.resources_only:
        return
    nat = native.load(required=True)
    tl = ["Factor imputation (k_ximp_gram, k_ximp_fill) on an MI355X next to a torch route on the same GPU",
          f"(tools/impute_profile.py; device events, median / min of {a.repeats} warm repeats, {min(a.repeats, 3)} for the torch route; XIMP_RUN {nat.ximp_run()}, "
          f"factors {a.factors}, ridge {GAMMA}).", ""]
    for label in PANELS:
        tl += time_panel(label, a.repeats, a.factors)
    with open(os.path.join(a.out_dir, "ximpute_timing.txt"), "w") as f:
        f.write("\n".join(tl) + "\n")
    print("\n".join(tl))


if __name__ == "__main__":
    main()
