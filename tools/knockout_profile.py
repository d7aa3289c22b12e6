"""Timing and accuracy of ``Engine.knockout`` (profiles/knockout_timing.txt, profiles/knockout_accuracy.txt).

    python tools/knockout_profile.py [--out-dir profiles]       # on the GPU
    python tools/knockout_profile.py --resources-only           # no GPU: appends the code-object section

Timing, on the bench panel's test split (300 x 3000 x 46 of the 600-month panel, M = 178, 9 members,
bf16), 47 + 6 scenarios (the baseline, every characteristic, six groups of consecutive columns):
1. ``Engine.knockout`` (refresh=False): GPU time of k_knock_fwd and k_knock_reduce from events around
   each, a warm-up call then ``--repeats`` calls; the cost per scenario.
2. The same scenarios the way the engine offered before: overwrite the columns of the batch,
   ``set_data``, ``forward_split``, read every member's weights back, average / re-normalise / Sharpe /
   EV on the host -- a host clock around the whole loop, ending in a device synchronise.
3. ``forward_split`` alone K times on the resident panel (events around the K calls): the floor of a
   tower recomputed per scenario; the ratio of 1 to it.
4. Registers, scratch and LDS of both kernels from the compiler's resource report of the code object.

Accuracy, on a smaller split (``--acc-T`` x ``--acc-N``; the float64 CPU path is the slow part): the fp32
engine against the float64 CPU path, the bf16 engine against the fp32 engine (Sharpe, EV, ranking)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    return f"median {statistics.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  (n = {len(ms)})"


def resources():
    """The compiler's resource report of csrc/k_knock.hip for gfx950, one line per kernel."""
    from deeplearninginassetpricing_paperreplication_amd.engine.build import ARCH, CSRC, HIPCC
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", f"-I{CSRC}",
                            "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "k_knock.hip"), "-o",
                            os.path.join(d, "k.o")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    lines, cur = [], {}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)}
            lines.append(cur)
        else:
            cur[m.group(1).split(" [")[0]] = m.group(2)
    out = ["Code object (hipcc -O3, gfx950; LDS is dynamic: the launch's image, at most 160 KiB for k_knock_fwd,",
           "4 x 5 doubles + 2 G floats for k_knock_reduce):"]
    for c in lines:
        name = re.sub(r"\(anonymous namespace\)::", "", c["name"]).split("(")[0]
        out.append(f"  {name:<36s} VGPRs {c.get('VGPRs'):>3s}  AGPRs {c.get('AGPRs'):>3s}  scratch {c.get('ScratchSize')} B/lane  "
                   f"VGPR spills {c.get('VGPRs Spill')}  SGPR spills {c.get('SGPRs Spill')}  occupancy {c.get('Occupancy')} waves/SIMD")
    spill = any(c.get("ScratchSize") != "0" or c.get("VGPRs Spill") != "0" for c in lines)
    out.append("  k_knock_fwd spills to scratch." if spill else
               "  No kernel uses scratch; the SGPR spills go to VGPR lanes (no memory traffic).")
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out-dir", type=str, default=os.path.join(ROOT, "profiles"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--G", type=int, default=9)
    p.add_argument("--acc-T", type=int, default=60)
    p.add_argument("--acc-N", type=int, default=1000)
    p.add_argument("--resources-only", action="store_true")
    p.add_argument("--skip-resources", action="store_true")
    a = p.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    tfile = os.path.join(a.out_dir, "knockout_timing.txt")
    if a.resources_only:
        with open(tfile, "a") as fh:
            fh.write("\n" + "\n".join(resources()) + "\n")
        return

    import torch
    import bench
    from deeplearninginassetpricing_paperreplication_amd.analysis import knockout as ko
    from deeplearninginassetpricing_paperreplication_amd.analysis.portfolio import (average_weights, explained_variation,
                                                                                     portfolio_returns, sharpe_ddof0)
    from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN
    if not torch.cuda.is_available():
        raise SystemExit("knockout_profile: no GPU")
    pc = bench.BENCH
    F, G = pc["F"], a.G
    test = bench.make_panel(0, "cuda", keep_on_device=True)[2]
    T, N = test["mask"].shape
    cfg = default_cli_config(pc["M"], F)
    models = []
    for g in range(G):
        torch.manual_seed(100 + g)
        models.append(AssetPricingGAN(cfg).eval())
    groups = {f"g{j}": list(range(8 * j, min(8 * j + 8, F))) for j in range(6)}
    labels, cols = ko.build_scenarios(F, groups)
    K = len(cols)
    b32 = [0.0] * F

    def engine(b, precision="bf16", ms=models):
        eng = GANEngine(ms[0].spec, len(ms), max_epochs=4, precision=precision)
        eng.set_data(b)
        for g, m in enumerate(ms):
            eng.set_model(g, m, 0)
        return eng

    out = [f"Engine.knockout on the bench panel's test split: T {T}, N {N}, F {F}, M {pc['M']}, G {G}, bf16, "
           f"K = {K} scenarios (baseline, {F} characteristics, {len(groups)} groups of 8 / 6 columns)"]
    eng = engine(test)
    e = eng.eng
    R = int(e.split_rows(0))
    e.forward_split(0, False, False)
    masks = ko.scenario_masks(cols, F)
    fw, rd = [], []
    for i in range(a.repeats + 1):
        r = e.knockout(0, masks, K, b32, 0, False)
        fw.append(float(r["fwd_ms"])); rd.append(float(r["reduce_ms"]))
    fw, rd = fw[1:], rd[1:]
    tot = statistics.median(fw) + statistics.median(rd)
    out += [f"1. rows {R}, {int(r['chunks'])} chunks ({K * G * R * 4 / 2 ** 20:.0f} MiB of raw weights in all, at most 256 MiB at a time)",
            f"   k_knock_fwd     {_stats(fw)}",
            f"   k_knock_reduce  {_stats(rd)}",
            f"   per scenario    {tot / K:.3f} ms ({statistics.median(fw) / K:.3f} forward + {statistics.median(rd) / K:.3f} reduce); "
            f"{K * G * R / statistics.median(fw) / 1e6:.2f}e9 tower evaluations / s"]
    sums = {k: np.asarray(r[k]) for k in ("n", "sum_r", "sum_rr") + ko.SUM_KEYS}
    met = ko.metrics_from_knockout_sums(sums)

    # 3. the floor: forward_split alone K times on the resident panel
    es = torch.cuda.ExternalStream(e.stream())
    fl = []
    for i in range(3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(es)
        for k in range(K):
            e.forward_split(0, False, False, False)
        ev[1].record(es)
        e.sync()
        fl.append(ev[0].elapsed_time(ev[1]))
    fl = fl[1:]

    # 2. the parent's route, end to end
    ret_np, mask_np = test["returns"].cpu().numpy(), test["mask"].cpu().numpy()

    def parent(ks):
        sh, evs = [], []
        for k in ks:
            b = dict(test)
            if len(cols[k]):
                x = test["individual_features"].clone()
                x[:, :, list(cols[k])] = 0.0
                b["individual_features"] = x
            eng.set_data(b)
            e.forward_split(0, False, False)
            ws = []
            for g in range(G):
                wn = np.asarray(e.read_ws(g, 0, "wn"))[:T * N].reshape(T, N)
                ws.append(wn / np.maximum(np.abs(wn * mask_np).sum(1, keepdims=True), 1e-8))
            avg = average_weights(ws, mask_np)
            sh.append(sharpe_ddof0(-portfolio_returns(avg, ret_np, mask_np).astype(np.float64)))
            evs.append(explained_variation(avg, ret_np, mask_np))
        e.sync()
        return np.array(sh), np.array(evs)

    parent([0])                                            # warm-up
    t0 = time.perf_counter()
    psh, pev = parent(range(K))
    t_parent = (time.perf_counter() - t0) * 1e3
    out += [f"2. the parent's route (overwrite, set_data, forward_split, read {G} x [T][N] weights, host metrics), "
            f"{K} scenarios end to end: {t_parent:.1f} ms = {t_parent / K:.2f} ms per scenario (one run, host clock); "
            f"knockout / parent = {tot / t_parent:.4f}",
            f"   agreement of the two routes: max |d Sharpe| {np.abs(psh - met['sharpe']).max():.2e}, "
            f"max |d EV| {np.abs(pev - met['ev']).max():.2e}",
            f"3. forward_split alone x {K} on the resident panel (LSTM prologue, tower forward, per-period "
            f"bookkeeping): {_stats(fl)}; knockout / floor = {tot / statistics.median(fl):.2f}, "
            f"k_knock_fwd / floor = {statistics.median(fw) / statistics.median(fl):.2f}"]
    del eng, e
    with open(tfile, "w") as fh:
        fh.write("\n".join(out) + "\n")
        if not a.skip_resources:
            fh.write("\n" + "\n".join(resources()) + "\n")
    print("\n".join(out))

    # ---- accuracy -----------------------------------------------------------------------------
    small = {k: v[:a.acc_T, :a.acc_N].contiguous() if k != "macro_features" else v[:a.acc_T].contiguous()
             for k, v in test.items()}
    cpu = {k: v.cpu() for k, v in small.items()}
    kw = dict(groups=groups, xs_r2=True)
    r64 = ko.knockout_importance(models, cpu, dtype=torch.float64, **kw)
    r32 = ko.knockout_importance(models, small, device="cuda", precision="fp32", **kw)
    r16 = ko.knockout_importance(models, small, device="cuda", precision="bf16", **kw)
    assert r32["path"] == r16["path"] == "engine"

    def rank_corr(x, y):
        rx, ry = np.argsort(np.argsort(x)).astype(float), np.argsort(np.argsort(y)).astype(float)
        return float(np.corrcoef(rx, ry)[0, 1])

    def cmp(x, y):
        sc = np.abs(y["factor"]).max()
        top = len(set(x["ranking"][:10]) & set(y["ranking"][:10]))
        return (f"max |dF| / max |F| {np.abs(x['factor'] - y['factor']).max() / sc:.3e}; "
                f"max |d Sharpe| {np.abs(x['sharpe'] - y['sharpe']).max():.3e}; max |d EV| {np.abs(x['ev'] - y['ev']).max():.3e}; "
                f"max |d XS-R2| {np.abs(x['xs_r2'] - y['xs_r2']).max():.3e}; "
                f"Spearman of d_sharpe {rank_corr(x['d_sharpe'][1:], y['d_sharpe'][1:]):.4f}; "
                f"top-10 by Sharpe loss shared {top} / 10")
    acc = [f"Knock-out accuracy: the first {a.acc_T} x {a.acc_N} of the bench test split, F {F}, G {G}, K = {K} scenarios, "
           f"untrained members (seeds 100..); baseline Sharpe {r64['sharpe'][0]:.4f}, EV {r64['ev'][0]:.4f}, "
           f"largest |d Sharpe| of a scenario {np.abs(r64['d_sharpe']).max():.4f}",
           f"fp32 engine against the float64 CPU path:  {cmp(r32, r64)}",
           f"bf16 engine against the fp32 engine:       {cmp(r16, r32)}",
           f"bf16 engine against the float64 CPU path:  {cmp(r16, r64)}"]
    with open(os.path.join(a.out_dir, "knockout_accuracy.txt"), "w") as fh:
        fh.write("\n".join(acc) + "\n")
    print("\n".join(acc))


if __name__ == "__main__":
    main()
