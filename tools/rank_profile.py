"""Timing, memory and kernel resources of the cross-sectional rank transform (``csrc/k_xrank.hip``):
writes ``rank_transform_timing.txt`` and ``rank_transform_resources.txt`` into ``--out_dir``.

    python tools/rank_profile.py [--out_dir profiles] [--repeats 9]

GPU only. Two raw panels (log-normal levels, 2 % of the entries -99.99, 0.5 % NaN, a tenth of the rows
dead; seeded, generated on the device): the three bench splits 240 / 60 / 300 x 3000 x 46 and one
16-period chunk of 30000 x 512 (0.98 GB). Per panel:
  kernel   ``_dlap_hip.rank_characteristics`` out of place into a buffer allocated before the window,
           device events around the launch, median / min of the warm repeats; GB/s = (x read + out
           written + rowok) / time;
  numpy    ``rank_characteristics_numpy`` on the host, a host clock around a few periods, scaled to
           the panel (marked as such);
  torch    a route that lives here only, on the same GPU: a transposed copy [T][F][N] with the
           non-participants set to +inf (the tool's panels hold no +inf of their own), ``torch.sort``
           along the stocks and two ``searchsorted``; events around the whole route.
For the kernel (in place, as ``rank_characteristics(x, rowok, out=x)`` runs it) and the torch route
the peak extra device memory is the ``torch.cuda.max_memory_allocated`` delta over the call. The
tool also checks that all three give the same bits. Resources: ``hipcc
-Rpass-analysis=kernel-resource-usage`` of the kernel file."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearninginassetpricing_paperreplication_amd.data import transforms as tr  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.dataset import MISSING_VALUE  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.ops import native  # noqa: E402

# label: (N, F, periods of each timed piece, periods the numpy definition is timed on)
PANELS = {"bench": (3000, 46, (240, 60, 300), 8), "scaled": (30000, 512, (16,), 1)}


def raw_panel(T, N, F, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((T, N, F), generator=g, device="cuda")
    x.mul_(1.5).exp_()
    u = torch.rand((T, N, F), generator=g, device="cuda")
    x[u < 0.02] = MISSING_VALUE
    x[u > 0.995] = float("nan")
    del u
    ok = (torch.rand((T, N), generator=g, device="cuda") > 0.1).to(torch.uint8)
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


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return out, peak


def torch_route(x, ok, fill_missing=0.0, fill_dead=MISSING_VALUE):
    thr = float(tr.THR)
    xt = x.transpose(1, 2).contiguous()                                   # [T][F][N]
    part = (xt > thr) & ok.bool()[:, None, :]
    xt = torch.where(part, xt, torch.full_like(xt, float("inf")))
    s = torch.sort(xt, dim=2).values
    m = part.sum(dim=2, keepdim=True)
    k = torch.searchsorted(s, xt, right=False) + torch.searchsorted(s, xt, right=True) - m
    y = k.to(torch.float32) / (2 * m).to(torch.float32)
    base = torch.where(ok.bool(), fill_missing, fill_dead).to(torch.float32)[:, None, :]
    y = torch.where(part, y, base.expand_as(y))
    return y.transpose(1, 2).contiguous(), m[:, :, 0].to(torch.int32)


def time_panel(label, repeats):
    nat = native.load(required=True)
    N, F, pieces, Tnp = PANELS[label]
    stream = torch.cuda.current_stream().cuda_stream
    thr = float(tr.THR)
    out = []
    for i, T in enumerate(pieces):
        x, ok = raw_panel(T, N, F, seed=100 + i)
        y = torch.empty_like(x)
        cnt = torch.empty((T, F), dtype=torch.int32, device="cuda")
        by = 2 * x.numel() * 4 + ok.numel()
        run = lambda: nat.rank_characteristics(x.data_ptr(), ok.data_ptr(), y.data_ptr(), cnt.data_ptr(), T, N, F,  # noqa: E731
                                               thr, 0.0, MISSING_VALUE, stream)
        md, mn = _events(run, repeats)
        tmd, tmn = _events(lambda: torch_route(x, ok), repeats)
        (ty, tc), tpeak = _peak(lambda: torch_route(x, ok))
        same_torch = torch.equal(ty.view(torch.int32), y.view(torch.int32)) and torch.equal(tc, cnt)
        del ty, tc
        xc = x.clone()
        (_, c2), kpeak = _peak(lambda: tr.rank_characteristics(xc, ok, out=xc))
        same_inplace = torch.equal(xc.view(torch.int32), y.view(torch.int32)) and torch.equal(c2, cnt)
        del xc, c2
        xh, okh = x[:Tnp].cpu().numpy(), ok[:Tnp].cpu().numpy().astype(bool)
        t0 = time.perf_counter()
        ny, nc = tr.rank_characteristics_numpy(xh, okh)
        tnp = (time.perf_counter() - t0) * 1e3
        same_np = (ny.view(np.uint32) == y[:Tnp].cpu().numpy().view(np.uint32)).all() and (nc == cnt[:Tnp].cpu().numpy()).all()
        out.append(f"  {label:<6s} {T:3d} x {N} x {F} ({x.numel() * 4 / 1e6:7.1f} MB)  k_xrank gpu_ms {md:9.3f} / {mn:9.3f}  "
                   f"{by / md / 1e6:7.1f} GB/s  peak extra {kpeak / 1e6:8.3f} MB   torch route ms {tmd:9.3f} / {tmn:9.3f}  "
                   f"peak extra {tpeak / 1e6:9.1f} MB   torch / kernel {tmd / md:6.2f}   numpy {tnp / Tnp:9.1f} ms per period "
                   f"({Tnp} timed) -> {tnp / Tnp * T / 1e3:8.2f} s scaled to {T}   numpy / kernel {tnp / Tnp * T / md:9.0f}   "
                   f"bits: in place {'same' if same_inplace else 'DIFFER'}, torch {'same' if same_torch else 'DIFFER'}, "
                   f"numpy {'same' if same_np else 'DIFFER'}")
        del x, ok, y, cnt
        torch.cuda.empty_cache()
    return out


def resources():
    """VGPRs, AGPRs, scratch, spills, occupancy of k_xrank from the compiler's remarks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "csrc", "k_xrank.hip")
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
    out = ["  kernel    SGPRs  VGPRs  AGPRs  scratch B/lane  VGPR spills  SGPR spills  waves/SIMD  static LDS B"]
    for c in rows:
        out.append(f"  {'k_xrank':<8s} {c.get('TotalSGPRs', -1):6d} {c.get('VGPRs', -1):6d} {c.get('AGPRs', -1):6d}  "
                   f"{c.get('ScratchSize', -1):14d}  {c.get('VGPRs Spill', -1):11d}  {c.get('SGPRs Spill', -1):11d}  "
                   f"{c.get('Occupancy', -1):10d}  {c.get('LDS Size', -1):12d}")
    return out


def kernel_rows(label, repeats):
    """The k_xrank timing of a panel's pieces alone (a side build's rows)."""
    nat = native.load(required=True)
    N, F, pieces, _ = PANELS[label]
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for i, T in enumerate(pieces):
        x, ok = raw_panel(T, N, F, seed=100 + i)
        y = torch.empty_like(x)
        cnt = torch.empty((T, F), dtype=torch.int32, device="cuda")
        md, mn = _events(lambda: nat.rank_characteristics(x.data_ptr(), ok.data_ptr(), y.data_ptr(), cnt.data_ptr(), T, N, F,
                                                          float(tr.THR), 0.0, MISSING_VALUE, stream), repeats)
        cb, P, nt, lds = launch_shape(N, F, nat.rank_block_keys())
        out.append(f"  {label:<6s} {T:3d} x {N} x {F}  XRANK_BLOCK_KEYS {nat.rank_block_keys():5d} ({cb} x {P} keys, {nt} threads, "
                   f"{lds} B LDS)  k_xrank gpu_ms {md:9.3f} / {mn:9.3f}")
        del x, ok, y, cnt
    return out


def launch_shape(N, F, block_keys=8192):
    """The launcher's choice for (N, F) (csrc/k_xrank.hip, launch_xrank)."""
    lp, fp2 = max(3, (N - 1).bit_length()), 1 << (F - 1).bit_length()
    lcb = 0
    while (2 << lcb) <= 8 and (2 << lcb) <= fp2 and ((2 << lcb) << lp) <= block_keys:
        lcb += 1
    tot = (1 << lcb) << lp
    nt = min(1024, max(64, (tot // 16 + 63) // 64 * 64))
    return 1 << lcb, 1 << lp, nt, (tot + (1 << lcb)) * 4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out_dir", type=str, default=os.path.join(ROOT, "profiles"))
    p.add_argument("--panels", nargs="+", default=list(PANELS))
    p.add_argument("--variants", type=str, nargs="*", default=[], help="side builds to time (DLAP_NATIVE names)")
    p.add_argument("--kernel_rows", action="store_true", help="print the k_xrank timing lines only (used for --variants)")
    a = p.parse_args()
    if a.repeats < 7:
        raise SystemExit("at least 7 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("rank_profile.py measures on the GPU: no GPU found")
    if a.kernel_rows:
        for label in a.panels:
            print("\n".join(kernel_rows(label, a.repeats)), flush=True)
        return
    os.makedirs(a.out_dir, exist_ok=True)
    tl = ["Rank transform (k_xrank) on an MI355X, next to the numpy definition on the host and a torch route on the same GPU",
          f"(transposed copy, torch.sort along the stocks, two searchsorted). gpu_ms / ms = device events, median / min of {a.repeats}",
          "warm repeats; numpy = a host clock around a few periods, scaled to the panel; peak extra = max_memory_allocated delta",
          "over one call (kernel: in place, rank_characteristics(x, rowok, out=x)). GB/s = (x + out + rowok) / gpu_ms.",
          "  python tools/rank_profile.py" + (" --variants " + " ".join(a.variants) if a.variants else ""), ""]
    for label in a.panels:
        tl += time_panel(label, a.repeats)
        tl.append("")
    for v in ([""] + a.variants) if a.variants else []:     # production again, then the side builds: one child process each
        env = dict(os.environ, DLAP_NATIVE=v)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel_rows", "--repeats", str(a.repeats), "--panels",
                            "bench"], env=env, capture_output=True, text=True, timeout=300)
        tl.append(f"side build {v} (DLAP_NATIVE={v}):" if v else "production build, kernel alone:")
        tl += [ln for ln in r.stdout.splitlines() if "k_xrank" in ln] if r.returncode == 0 else [f"  (failed: {r.stderr[-300:]})"]
        tl.append("")
    rl = ["Kernel resources of k_xrank (gfx950, -O3; hipcc -Rpass-analysis=kernel-resource-usage). N and F are run-time",
          "arguments and the LDS is dynamic, sized by the launcher:"] + resources() + [""]
    for N, F in ((1000, 46), (3000, 46), (30000, 512), (32768, 1)):
        cb, P, nt, lds = launch_shape(N, F)
        rl.append(f"  N = {N:5d}, F = {F:3d}: {cb} column(s) of {P} keys per workgroup, {nt} threads, {lds} B of LDS "
                  f"({min(163840 // lds, 2048 // nt)} workgroup(s) per CU)")
    for name, lines in (("rank_transform_timing.txt", tl), ("rank_transform_resources.txt", rl)):
        with open(os.path.join(a.out_dir, name), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
