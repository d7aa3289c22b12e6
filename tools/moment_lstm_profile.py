"""Timing of the moment network's own macro LSTM (config key ``moment_lstm``) on one MI355X.

Bench panel (600 x 3000 x 46, M = 178, splits 240 / 60 / 300), bf16 engine, one model and 8 batched,
CSMV off / 16 / 32:

  * steady phase-2 ms per epoch (graph replay, host clock around a device synchronise; warm-up, then
    ``--repeats`` windows of ``--epochs`` epochs: median and range);
  * the first phase-3 call after phase 2 (one epoch: the moment refresh of the three splits, the
    Gram builds and the head epoch), against the same call without the LSTM;
  * one 4-member paper-grid bucket (HL 2 / SMV 4 / CHL 0 / CHU 8) with the flag: ms per epoch per phase.

``--trace full|short|tiny``: the workload for a ``rocprofv3 --kernel-trace --stats`` run of its own (no
timing): phase-2 epochs with CSMV 16 and 32, and, as the baseline of the new recurrence and BPTT, the
existing generic kernels driven as an SDF LSTM of the same width (``num_units_rnn`` [16] / [32]) on the
same train split (see ``trace``). Summarise the trace with tools/kernel_stats.py.

Usage (GPU box): python tools/moment_lstm_profile.py [--out FILE] | --trace full | short | tiny
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _engine(cfg, G, tr, va, te, max_epochs):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN
    torch.manual_seed(0)
    models = [AssetPricingGAN(cfg) for _ in range(G)]
    eng = GANEngine(models[0].spec, G, max_epochs=max_epochs)
    eng.set_data(tr, va, te)
    for g, m in enumerate(models):
        eng.set_model(g, m, g + 1)
    return eng


def _timed(eng, phase, n):
    eng.eng.sync()
    t0 = time.perf_counter()
    eng.run(phase, n, 1e-3, 0)
    eng.eng.sync()
    return (time.perf_counter() - t0) / n * 1e3


def _cfg(csmv, **kw):
    from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
    import bench
    return default_cli_config(bench.BENCH["M"], bench.BENCH["F"], rnn_dim_moment=[csmv or 32],
                              moment_lstm=bool(csmv), **kw)


def timing(a, say):
    import bench
    tr, va, te = bench.make_panel(seed=0, device="cuda")
    n, reps = a.epochs, a.repeats
    say(f"device: {torch.cuda.get_device_name(0)}; bench panel 600 x 3000 x 46, M = 178, bf16 engine")
    say(f"phase 2: {reps} windows of {n} epochs after a {n}-epoch warm-up; ms per epoch, median [min, max]")
    say("first phase-3 call: begin_phase(3) + 1 epoch right after phase 2 (refresh of the three splits, Gram "
        "builds, head epoch), median of 3 alternations with phase 2")
    for G in (1, 8):
        for csmv in (0, 16, 32):
            eng = _engine(_cfg(csmv), G, tr, va, te, 8 * n * (reps + 2))
            for ph in (1, 2, 3, 2):                    # graph capture of every phase, warm-up
                eng.eng.begin_phase(ph)
                eng.run(ph, n if ph == 2 else 4, 1e-3, 0)
            w = [_timed(eng, 2, n) for _ in range(reps)]
            first3 = []
            for _ in range(3):
                eng.eng.begin_phase(2)
                eng.run(2, 4, 1e-3, 0)
                eng.eng.sync()
                t0 = time.perf_counter()
                eng.eng.begin_phase(3)
                eng.run(3, 1, 1e-3, 0)
                eng.eng.sync()
                first3.append((time.perf_counter() - t0) * 1e3)
            info = eng.eng.fused_info()
            say(f"G={G} CSMV={'off' if not csmv else csmv:>3}: phase 2 {statistics.median(w):.4f} "
                f"[{min(w):.4f}, {max(w):.4f}] ms/epoch  mom_tail={info['mom_tail']}  "
                f"first phase-3 call {statistics.median(first3):.3f} ms")
            del eng
            torch.cuda.empty_cache()
    say("sweep bucket HL 2 / SMV 4 / CHL 0 / CHU 8 with --moment_lstm (4 members: the LR axis), ms per epoch")
    for csmv in (16, 32):
        eng = _engine(_cfg(csmv, hidden_dim=[64, 64], rnn_dim=[4], num_moments=8), 4, tr, va, te, 16 * n)
        for ph in (1, 2, 3):
            eng.eng.begin_phase(ph)
            eng.run(ph, 4, 1e-3, 0)
        per = []
        for ph in (1, 2, 3):
            eng.eng.begin_phase(ph)
            per.append(_timed(eng, ph, n))
        say(f"CSMV={csmv}: phase 1 {per[0]:.4f}  phase 2 {per[1]:.4f}  phase 3 {per[2]:.4f}  "
            f"schedule-weighted (256:64:1024) {(256 * per[0] + 64 * per[1] + 1024 * per[2]) / 1344:.4f}")
        del eng
        torch.cuda.empty_cache()


def trace(a):
    """``full``: the bench panel's train split (T = 240): phase-2 epochs with CSMV 16 / 32 (k_mlstm_*), and the
    generic recurrence kernels (k_lstm_gl<16> / k_lstm<32>) as an SDF LSTM of the same width through the
    evaluation forward. The generic BPTT kernels stage T x 12 H floats plus their weight-gradient
    partials in LDS and refuse T = 240 at these widths (k_lstm_bwd<16>: T <= 163, k_lstm_bwd<32>: T <= 16),
    so ``short`` compares width 16 at 100 train periods and ``tiny`` width 32 at 16: phase-1 epochs with
    the separate launches (safe mode) against phase-2 epochs of the new kernels."""
    import bench
    t_train, widths = {"full": (240, (16, 32)), "short": (100, (16,)), "tiny": (16, (32,))}[a.trace]
    tr = bench.make_panel(seed=0, device="cuda", cfg=dict(bench.BENCH, T_train=t_train))[0]
    n = 40
    for csmv in widths:                              # the new kernels: k_mlstm_*
        eng = _engine(_cfg(csmv), 1, tr, None, None, 8 * n)
        eng.eng.begin_phase(2)
        eng.run(2, n, 1e-3, 0)
        eng.eng.sync()
        del eng
    for h in widths:                                   # the baseline: the generic SDF LSTM kernels
        eng = _engine(_cfg(0, rnn_dim=[h]), 1, tr, None, None, 8 * n)
        eng.eng.set_safe_mode(True)                    # separate recurrence / BPTT launches
        if a.trace == "full":
            for _ in range(n):
                eng.eng.forward_split(0, False, False)
        else:
            eng.eng.begin_phase(1)
            eng.run(1, n, 1e-3, 0)
        eng.eng.sync()
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", choices=["full", "short", "tiny"], default=None)
    ap.add_argument("--epochs", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moment_lstm_profile needs a GPU")
    torch.cuda.set_device(0)
    if a.trace:
        trace(a)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    timing(a, say)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
