"""Timing and accuracy of the prediction towers (``csrc/k_pred.hip``, ``Engine.fit_epochs``,
``analysis.prediction``): writes ``prediction_timing.txt`` and ``prediction_accuracy.txt`` into
``--out_dir``.

    python tools/prediction_profile.py [--out_dir profiles]        # bench panel 600 x 3000 x 46, M = 178
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prediction_profile.py --trace_run 9
                                                                   # per-kernel split of the fit epoch, a run of its own

GPU only. Timing: per G (1 and 9 batched seeds, bf16) the wall time per fit epoch of
``fit_epochs(n)`` + one synchronisation (median / min of the repeats), the host time the enqueue
takes (the epoch is ungraphed and single-stream), and next to it the phase-1 GAN epoch of the same
engine (``run_epochs``: graphed, pipelined), the number ``bench.py`` is built on. Accuracy (dropout
0, so both devices draw no masks): the bf16 and the fp32 engine against the fp32 torch loop --
predictions, FFN Sharpe / EV / XS-R2 and beta-network EV / XS-R2."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BENCH, make_panel  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.analysis import prediction as pr  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN  # noqa: E402


def _engine(cfg, splits, G, max_epochs=4096):
    models = []
    for g in range(G):
        torch.manual_seed(g)
        models.append(AssetPricingGAN(cfg))
    eng = GANEngine(models[0].spec, G, max_epochs=max_epochs)
    eng.set_data(*splits)
    for g, m in enumerate(models):
        eng.set_model(g, m, g)
    eng.eng.sync()
    return eng


def _time_fit(eng, n, repeats, lr):
    e = eng.eng
    e.fit_begin([None, None, None], "period")
    e.fit_epochs(3, lr)
    e.sync()
    wall, host = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        e.fit_epochs(n, lr)
        t1 = time.perf_counter()
        e.sync()
        t2 = time.perf_counter()
        wall.append((t2 - t0) / n * 1e3)
        host.append((t1 - t0) / n * 1e3)
    assert e.prog_timeouts() == 0
    return wall, host


def _time_gan(eng, n, repeats, lr):
    e = eng.eng
    e.plan_phase(1, n * (repeats + 1))
    e.begin_phase(1)
    eng.run(1, n, lr, 0)
    e.sync()
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        eng.run(1, n, lr, 0)
        e.sync()
        wall.append((time.perf_counter() - t0) / n * 1e3)
    return wall


def trace_run(G, n, lr):
    cfg = default_cli_config(BENCH["M"], BENCH["F"])
    splits = make_panel(device="cuda", keep_on_device=True)
    eng = _engine(cfg, splits, G)
    e = eng.eng
    e.fit_begin([None, None, None], "period")
    e.fit_epochs(n, lr)
    e.sync()
    print(f"trace run: {n} fit epochs, G = {G}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=50, help="fit epochs per timed repeat")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--accuracy_epochs", type=int, default=12)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--trace_run", type=int, default=0, metavar="G", help="only run --epochs fit epochs of G models (for rocprofv3)")
    p.add_argument("--skip_accuracy", action="store_true")
    p.add_argument("--out_dir", type=str, default=os.path.join(ROOT, "profiles"))
    a = p.parse_args()
    if a.trace_run:
        trace_run(a.trace_run, a.epochs, a.lr)
        return
    os.makedirs(a.out_dir, exist_ok=True)
    T = (BENCH["T_train"], BENCH["T_valid"], BENCH["T_test"])
    cfg = default_cli_config(BENCH["M"], BENCH["F"])
    splits = make_panel(device="cuda", keep_on_device=True)
    rows = [int(b["mask"].sum()) for b in splits]
    tl = ["Engine.fit_epochs (prediction towers: train forward, k_pred_loss, tower backward, tail, k_adam, evaluation towers,",
          "k_pred_loss x 2, k_pred_end) on an MI355X, bf16 panel, dropout 0.05, ungraphed, one stream",
          f"wall = fit_epochs({a.epochs}) + one synchronisation, per epoch; host = the enqueue alone; median / min of {a.repeats} repeats",
          "  python tools/prediction_profile.py", "",
          f"panel {sum(T)} x {BENCH['N']} x {BENCH['F']}, M = {BENCH['M']} (bench.py's), splits {T[0]} / {T[1]} / {T[2]} periods, "
          f"{rows[0]} / {rows[1]} / {rows[2]} valid rows", ""]
    for G in (1, 9):
        eng = _engine(cfg, splits, G)
        wall, host = _time_fit(eng, a.epochs, a.repeats, a.lr)
        del eng
        eng = _engine(cfg, splits, G)
        gan = _time_gan(eng, a.epochs, a.repeats, a.lr)
        del eng
        tl.append(f"  G = {G}  fit epoch   wall {statistics.median(wall):.4f} / {min(wall):.4f} ms   host enqueue "
                  f"{statistics.median(host):.4f} / {min(host):.4f} ms   ({G / statistics.median(wall) * 1e3:.0f} model-epochs/s)")
        tl.append(f"  G = {G}  phase-1 GAN epoch (run_epochs, graphed + pipelined, with its evaluation)   wall "
                  f"{statistics.median(gan):.4f} / {min(gan):.4f} ms   ({G / statistics.median(gan) * 1e3:.0f} model-epochs/s)")
    with open(os.path.join(a.out_dir, "prediction_timing.txt"), "w") as fh:
        fh.write("\n".join(tl) + "\n")
    print("\n".join(tl), flush=True)
    if a.skip_accuracy:
        return
    # accuracy: dropout 0, one seed, the three executors on the same panel
    cfg0 = default_cli_config(BENCH["M"], BENCH["F"], dropout=0.0)
    names = pr.SPLITS
    host = {s: {k: v.cpu() for k, v in b.items()} for s, b in zip(names, splits)}
    kw = dict(epochs=a.accuracy_epochs, lr=a.lr, seeds=(0,))
    res = {}
    for tag, dev, prec in (("cpu fp32", "cpu", "fp32"), ("gpu fp32", "cuda", "fp32"), ("gpu bf16", "cuda", "bf16")):
        t0 = time.perf_counter()
        ffn = pr.ffn_benchmark(host, cfg0, device=dev, precision=prec, **kw)
        beta = pr.beta_network(ffn["weights"] if tag == "cpu fp32" else res["cpu fp32"][0]["weights"], host, cfg0,
                               device=dev, precision=prec, **kw)
        res[tag] = (ffn, beta, time.perf_counter() - t0)
    al = ["Prediction towers: the GPU engines against the fp32 torch loop (analysis.prediction, device='cpu') on an MI355X",
          f"bench panel {sum(T)} x {BENCH['N']} x {BENCH['F']}, M = {BENCH['M']}; dropout 0 (no masks on either device), 1 seed, "
          f"{a.accuracy_epochs} epochs, lr {a.lr:g}; the beta network's factor comes from the CPU FFN weights for all three",
          "  python tools/prediction_profile.py", ""]
    fc, bc, tc = res["cpu fp32"]
    al.append(f"  cpu fp32: FFN + beta network in {tc:.1f} s; FFN Sharpe train/valid/test "
              + " / ".join(f"{fc['sharpe'][s]:.4f}" for s in names) + f", EV test {fc['ev']['test']:.4f}, XS-R2 test {fc['xs_r2']['test']:.4f}; "
              f"beta net EV test {bc['ev']['test']:.4f}, XS-R2 test {bc['xs_r2']['test']:.4f}")
    for tag in ("gpu fp32", "gpu bf16"):
        f, b, t = res[tag]
        al.append(f"  {tag}: FFN + beta network in {t:.1f} s")
        hrel = np.abs(np.asarray(f["history"][0], np.float64)[:, :4] - np.asarray(fc["history"][0], np.float64)[:, :4]) / \
            np.abs(np.asarray(fc["history"][0], np.float64)[:, :4])
        al.append(f"    FFN history (train, valid, test loss, grad norm): largest relative difference {hrel.max(axis=0)}")
        for s in names:
            m = host[s]["mask"].numpy()
            pc, pg = fc["weights"][s][m], f["weights"][s][m]
            al.append(f"    {s:<5s} FFN L1-normalised weights: max |d| / max |w| {np.abs(pg - pc).max() / np.abs(pc).max():.3e}   "
                      f"Sharpe d {f['sharpe'][s] - fc['sharpe'][s]:+.2e}  EV d {f['ev'][s] - fc['ev'][s]:+.2e}  "
                      f"XS-R2 d {f['xs_r2'][s] - fc['xs_r2'][s]:+.2e}")
            bcs, bgs = bc["beta"][s][m], b["beta"][s][m]
            al.append(f"    {s:<5s} beta: max |d| / max |beta| {np.abs(bgs - bcs).max() / np.abs(bcs).max():.3e}   "
                      f"EV d {b['ev'][s] - bc['ev'][s]:+.2e}  XS-R2 d {b['xs_r2'][s] - bc['xs_r2'][s]:+.2e}")
    with open(os.path.join(a.out_dir, "prediction_accuracy.txt"), "w") as fh:
        fh.write("\n".join(al) + "\n")
    print("\n".join(al), flush=True)


if __name__ == "__main__":
    main()
