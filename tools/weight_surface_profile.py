"""Timing of ``Engine.weight_surface`` (profiles/weight_surface_timing.txt).

    python tools/weight_surface_profile.py                 # bench shape: T 300, F 46, Dm 4, 9 models, bf16

1. Comparison with the only route the engine offered before: 46 curves + 10 surfaces at P = 21
   (5376 rows). Route A uploads a dense fake panel whose stocks are those rows in every period and
   runs ``forward_split`` of all models on it (events on the engine stream around the call: the
   LSTM prologue, the tower forward over T x 5376 rows per model and forward_split's per-period
   bookkeeping; the upload and the host-side sum over periods and models are left out). A0 is the
   same call on a fake panel of 32 rows: what of A does not depend on the rows. Route B is the
   k_wsurf launch alone (``gpu_ms``, refresh=False; its per-period inputs come from the forward of
   the real panel, which the scale table needs anyway). Warm-up call first, then ``--repeats``
   calls: median, min and max of each.
2. The full job: every pair (1035 surfaces) and every curve at P = 21 -- no baseline exists."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deeplearninginassetpricing_paperreplication_amd.analysis.weight_structure import make_rows  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN  # noqa: E402


def _stats(ms):
    return f"median {statistics.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  (n = {len(ms)})"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--T", type=int, default=300)
    p.add_argument("--N", type=int, default=3000)
    p.add_argument("--F", type=int, default=46)
    p.add_argument("--G", type=int, default=9)
    p.add_argument("--P", type=int, default=21)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--precision", type=str, default="bf16")
    p.add_argument("--skip-full", action="store_true")
    a = p.parse_args()
    T, N, F, G, P = a.T, a.N, a.F, a.G, a.P
    ret, feats, mask, mac = generate_panel_fast(T, N, F, 8, seed=0, device="cuda")
    batch = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    cfg = default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4])
    models = []
    for g in range(G):
        torch.manual_seed(100 + g)
        models.append(AssetPricingGAN(cfg).eval())
    grid = np.linspace(-0.45, 0.45, P).astype(np.float32)
    base = np.zeros(F, dtype=np.float32)
    g32, b32 = [float(x) for x in grid], [float(x) for x in base]
    curves = [(c, -1) for c in range(F)]
    some = curves + [(c, c + 1) for c in range(0, 20, 2)]
    every = curves + [(c, d) for c in range(F) for d in range(c + 1, F)]
    print(f"T {T}, F {F}, Dm 4, G {G}, P {P}, {a.precision}; real panel {T} x {N}")

    def engine(b):
        eng = GANEngine(models[0].spec, G, max_epochs=4, precision=a.precision)
        eng.set_data(b)
        for g, m in enumerate(models):
            eng.set_model(g, m, 0)
        return eng

    eng = engine(batch)
    e = eng.eng
    e.forward_split(0, False, False)                       # the per-period inputs are current from here on

    def run(items):
        ms = []
        for i in range(a.repeats + 1):
            r = e.weight_surface(0, 0, g32, b32, items, False)
            ms.append(float(r["gpu_ms"]))
        return ms[1:], r

    ms_b, r = run(some)
    rows = int(r["rows"])
    print(f"B  k_wsurf, {len(some)} items, {rows} rows, period split {r['period_split']}, tiles/wave {r['tiles_per_wave']}: {_stats(ms_b)}")
    vals_b = np.asarray(r["values"], dtype=np.float64)
    if not a.skip_full:
        ms_f, rf = run(every)
        print(f"   k_wsurf, full job {len(every)} items, {int(rf['rows'])} rows, period split {rf['period_split']}, tiles/wave {rf['tiles_per_wave']}: {_stats(ms_f)}")
        print(f"   = {int(rf['rows']) * T * G / 1e9:.3f}e9 tower evaluations, "
              f"{int(rf['rows']) * T * G / statistics.median(ms_f) / 1e6:.2f}e9 / s")
    del eng, e
    # route A: the rows as the stocks of a dense fake panel
    X = torch.as_tensor(make_rows(grid.astype(np.float64), base.astype(np.float64), [c for c, d in some if d < 0],
                                  [(c, d) for c, d in some if d >= 0]).astype(np.float32)).cuda()

    def route_a(n):
        fake = {"returns": torch.zeros(T, n, device="cuda"), "individual_features": X[None, :n].expand(T, n, F).contiguous(),
                "mask": torch.ones(T, n, dtype=torch.bool, device="cuda"), "macro_features": mac}
        eng = engine(fake)
        e = eng.eng
        es = torch.cuda.ExternalStream(e.stream())
        ms = []
        for i in range(a.repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(es)
            e.forward_split(0, False, False, False)
            ev[1].record(es)
            e.sync()
            ms.append(ev[0].elapsed_time(ev[1]))
        return ms[1:], eng

    ms_a0, eng = route_a(32)
    del eng
    print(f"A0 forward_split of {G} models on a fake panel {T} x 32 (LSTM prologue, per-period bookkeeping): {_stats(ms_a0)}")
    ms_a, eng = route_a(rows)
    e = eng.eng
    print(f"A  forward_split of {G} models on the fake panel {T} x {rows} ({T * rows * F * 4 / 1e6:.0f} MB dense fp32): {_stats(ms_a)}")
    w = np.stack([np.asarray(e.read_ws(g, 0, "w"), dtype=np.float64)[:T * rows].reshape(T, rows) for g in range(G)])
    diff = np.abs(w.sum((0, 1)) - vals_b).max() / np.abs(vals_b).max()
    print(f"   sum over models and periods of A's weights against B (scale ones): max-rel {diff:.2e}")
    spread = max(max(ms_a) - min(ms_a), max(ms_b) - min(ms_b))
    print(f"B / A = {statistics.median(ms_b) / statistics.median(ms_a):.2f} (medians); run-to-run spread (max - min) "
          f"A {max(ms_a) - min(ms_a):.3f} ms, B {max(ms_b) - min(ms_b):.3f} ms; "
          f"B - A = {statistics.median(ms_b) - statistics.median(ms_a):+.3f} ms against {spread:.3f} ms; "
          f"A - A0 = {statistics.median(ms_a) - statistics.median(ms_a0):.3f} ms")


if __name__ == "__main__":
    main()
