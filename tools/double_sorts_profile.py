"""Timing and bf16-membership figures of ``Engine.double_sorted_portfolios`` (profiles/double_sorts_*.txt).

    python tools/double_sorts_profile.py                       # bench panel 600 x 3000 x 46, its test split

GPU only. On the test split (the last 300 periods) of the generator panel, Qa x Qb = 5 x 5, return +
one value column (the evaluator's case), per mode and precision: the kernel time (``gpu_ms``, events
on the engine stream; median and min of the warm repeats) of one pair, of the 45 pairs with first key
0, and of 100 arbitrary pairs; beside it ``k_qsort_port``'s time for the same split and Q = 5 (one
column, and all 46 divided by 46) and the numpy path's wall time. With both precisions: the share of
rows whose cell differs between the bf16-stored and the fp32 keys, for a few pairs."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deeplearninginassetpricing_paperreplication_amd.analysis import sorted_portfolios as sp  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN  # noqa: E402


def _med(eng_call, repeats):
    ms = [float(eng_call()["gpu_ms"]) for _ in range(repeats + 1)]
    return statistics.median(ms[1:]), min(ms[1:]), ms[0]


def _cells(a, b, ba, bb):
    """cell index [T][N] of keys a, b [T][N] under breaks_a [T][Qa-1] and breaks_b [T][Qa][Qb-1]"""
    qa = (a[:, :, None] > ba[:, None, :]).sum(-1)
    sel = torch.gather(bb, 1, qa[:, :, None].expand(-1, -1, bb.shape[2]))
    qb = (b[:, :, None] > sel).sum(-1)
    return qa * (bb.shape[2] + 1) + qb


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--T", type=int, default=600)
    p.add_argument("--N", type=int, default=3000)
    p.add_argument("--F", type=int, default=46)
    p.add_argument("--test_from", type=int, default=300, help="first period of the test split")
    p.add_argument("--qa", type=int, default=5)
    p.add_argument("--qb", type=int, default=5)
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--numpy_pairs", type=int, default=3)
    a = p.parse_args()
    if a.repeats < 7:
        raise SystemExit("at least 7 repeats")
    dev = torch.device("cuda")
    T, N, F, Qa, Qb = a.T, a.N, a.F, a.qa, a.qb
    ret, feats, mask, mac = generate_panel_fast(T, N, F, 8, seed=0, device="cuda")
    s = slice(a.test_from, T)
    mac = (mac - mac[:a.test_from].mean(0)) / (mac[:a.test_from].std(0, unbiased=False) + 1e-8)
    batch = {"returns": ret[s].contiguous(), "individual_features": feats[s].contiguous(),
             "mask": mask[s].contiguous(), "macro_features": mac[s].contiguous()}
    Ts = T - a.test_from
    rows = int(batch["mask"].sum())
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(Ts, N, device=dev, generator=g).contiguous()        # the value column (a stand-in weight)
    rng = np.random.default_rng(0)
    one = [(3, 17)]
    fixed = [(0, b) for b in range(1, F)]
    arb = [tuple(int(x) for x in rng.integers(0, F, 2)) for _ in range(100)]
    spec = AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4])).spec
    print(f"panel {T} x {N} x {F} (generate_panel_fast), test split = periods {a.test_from}..{T - 1}: {Ts} periods, "
          f"{rows} valid rows; {Qa} x {Qb} cells, return + 1 value column, {a.repeats} warm repeats", flush=True)
    breaks = {}
    for prec in ("bf16", "fp32"):
        eng = GANEngine(spec, 1, max_epochs=4, precision=prec)
        eng.set_data(batch)
        torch.cuda.synchronize()
        e = eng.eng
        m1, n1, _ = _med(lambda: e.sorted_portfolios(0, Qa, [3], 0, 0, w.data_ptr(), 1), a.repeats)
        mF, nF, _ = _med(lambda: e.sorted_portfolios(0, Qa, [], 0, 0, w.data_ptr(), 1), a.repeats)
        print(f"  {prec}  k_qsort_port Q = {Qa}: one column {m1:.4f} / {n1:.4f} ms; all {F} columns {mF:.4f} / {nF:.4f} ms "
              f"= {mF / F:.4f} ms per key", flush=True)
        for cond in (True, False):
            mode = "conditional" if cond else "independent"
            res = {}
            for name, prs in (("1 pair", one), (f"{len(fixed)} pairs, first key 0", fixed), ("100 arbitrary pairs", arb)):
                md, mn, first = _med(lambda: e.double_sorted_portfolios(0, prs, Qa, Qb, cond, 0, 0, w.data_ptr(), 1), a.repeats)
                res[name] = md
                print(f"  {prec}  {mode:<11s} {name:<26s} gpu_ms {md:.4f} / {mn:.4f} (first call {first:.4f}) "
                      f"= {md / len(prs):.4f} ms per pair = {md / len(prs) / (mF / F):.2f} x a single key in the {F}-column launch",
                      flush=True)
            print(f"  {prec}  {mode:<11s} one pair alone / one column alone = {res['1 pair'] / m1:.2f}", flush=True)
        r = e.double_sorted_portfolios(0, fixed[:8] + [(3, 17), (17, 3)], Qa, Qb, True)
        breaks[prec] = (torch.as_tensor(r["breaks_a"]).to(dev), torch.as_tensor(r["breaks_b"]).to(dev),
                        fixed[:8] + [(3, 17), (17, 3)])
        e.sync()
        del eng
    # numpy path (the definition) on the same split
    keys = batch["individual_features"].cpu().numpy().astype(np.float32)
    vals = np.stack([batch["returns"].cpu().numpy().astype(np.float32), w.cpu().numpy()], axis=2)
    mk = batch["mask"].cpu().numpy()
    for cond in (True, False):
        t0 = time.perf_counter()
        sp.double_sort_numpy(keys, fixed[:a.numpy_pairs], mk, vals, (Qa, Qb), cond)
        dt = time.perf_counter() - t0
        print(f"  numpy   {'conditional' if cond else 'independent':<11s} {a.numpy_pairs} pairs: {dt * 1e3:.0f} ms wall "
              f"= {dt * 1e3 / a.numpy_pairs:.0f} ms per pair", flush=True)
    # rows whose cell differs between the bf16-stored and the fp32 keys (conditional sort)
    ba16, bb16, prs = breaks["bf16"]
    ba32, bb32, _ = breaks["fp32"]
    x = batch["individual_features"]
    x16 = x.to(torch.bfloat16).float()
    m = batch["mask"]
    tot_d = tot_r = 0
    for i, (ca, cb) in enumerate(prs):
        c16 = _cells(x16[:, :, ca], x16[:, :, cb], ba16[:, i], bb16[:, i])
        c32 = _cells(x[:, :, ca], x[:, :, cb], ba32[:, i], bb32[:, i])
        d = int(((c16 != c32) & m).sum())
        tot_d += d
        tot_r += rows
        print(f"  pair ({ca}, {cb}): rows whose cell differs between bf16-stored and fp32 keys: {d} of {rows} = {100.0 * d / rows:.3f} %",
              flush=True)
    print(f"  all {len(prs)} pairs: {tot_d} of {tot_r} = {100.0 * tot_d / tot_r:.3f} %", flush=True)


if __name__ == "__main__":
    main()
