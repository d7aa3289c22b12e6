"""Timing and bf16-membership figures of ``Engine.sorted_portfolios`` (profiles/sorted_portfolios_*.txt).

    python tools/sorted_portfolios_profile.py --T 600 --N 3000 --F 46                  # bench panel
    python tools/sorted_portfolios_profile.py --T 600 --N 30000 --F 512 --randn        # scaled panel

Per precision: the kernel time (``gpu_ms``, events on the engine stream; median of the repeats) of
sorting every characteristic into deciles, beside ``torch.sort`` of the same keys as dense fp32
[T][F][N] rows on the GPU (in period chunks, the chunk times added up) and the time one read of the
resident panel ``X`` takes at the HBM rate a streaming kernel reaches on an MI355X (6.3 TB/s).
With both precisions: the share of rows whose bucket differs between the bf16-stored and the fp32
keys."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--T", type=int, default=600)
    p.add_argument("--N", type=int, default=3000)
    p.add_argument("--F", type=int, default=46)
    p.add_argument("--Q", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--precisions", type=str, default="bf16,fp32")
    p.add_argument("--randn", action="store_true", help="standard normal characteristics instead of the generator's")
    p.add_argument("--no-torch-sort", action="store_true")
    a = p.parse_args()
    dev = torch.device("cuda")
    T, N, F, Q = a.T, a.N, a.F, a.Q
    if a.randn:
        g = torch.Generator(device=dev).manual_seed(0)
        feats = torch.empty(T, N, F, device=dev)
        for t in range(T):
            feats[t] = torch.randn(N, F, device=dev, generator=g)
        ret = 0.1 * torch.randn(T, N, device=dev, generator=g)
        mask = torch.ones(T, N, dtype=torch.bool, device=dev)
        mac = torch.randn(T, 8, device=dev, generator=g)
    else:
        ret, feats, mask, mac = generate_panel_fast(T, N, F, 8, seed=0, device="cuda")
    batch = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    spec = AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4])).spec
    print(f"panel {T} x {N} x {F}, Q = {Q}, rows {int(mask.sum())}, {'randn' if a.randn else 'generate_panel_fast'} keys")
    breaks = {}
    for prec in a.precisions.split(","):
        eng = GANEngine(spec, 1, max_epochs=4, precision=prec)
        eng.set_data(batch)
        kp = int(eng.desc["KP"])
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats + 1):
            r = eng.eng.sorted_portfolios(0, Q)
            ms.append(float(r["gpu_ms"]))
        xbytes = int(r["rows"]) * kp * (4 if prec == "fp32" else 2)
        print(f"  {prec}: gpu_ms median {statistics.median(ms[1:]):.3f} min {min(ms[1:]):.3f} (first call {ms[0]:.3f}); "
              f"wide {int(eng.desc['wide'])}, KP {kp}, X {xbytes / 1e6:.1f} MB -> one read at 6.3 TB/s {xbytes / HBM_BYTES_PER_S * 1e3:.3f} ms")
        breaks[prec] = torch.as_tensor(r["breaks"]).to(dev)
        del eng
    if not a.no_torch_sort:
        chunk = max(1, (1 << 28) // (N * F))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rep in range(2):                              # (the second pass is the warm one)
            tot_s = tot_t = 0.0
            for t0 in range(0, T, chunk):
                x = feats[t0:t0 + chunk]
                ev[0].record()
                xt = x.transpose(1, 2).contiguous()
                ev[1].record()
                torch.cuda.synchronize()
                tot_t += ev[0].elapsed_time(ev[1])
                ev[0].record()
                torch.sort(xt, dim=2)
                ev[1].record()
                torch.cuda.synchronize()
                tot_s += ev[0].elapsed_time(ev[1])
                del xt
        print(f"  torch.sort of dense fp32 [T][F][N] keys (chunks of {chunk} periods): {tot_s:.3f} ms, "
              f"+ {tot_t:.3f} ms for the [T][N][F] -> [T][F][N] copy it needs; values and indices only, no bucket sums")
    if "bf16" in breaks and "fp32" in breaks:
        diff = rows = 0
        for t in range(T):
            x = feats[t]                                   # [N][F]
            b16 = (x.to(torch.bfloat16).float()[:, :, None] > breaks["bf16"][t][None]).sum(-1)
            b32 = (x[:, :, None] > breaks["fp32"][t][None]).sum(-1)
            m = mask[t][:, None]
            diff += int(((b16 != b32) & m).sum())
            rows += int(m.sum()) * F
        print(f"  rows whose bucket differs between bf16-stored and fp32 keys: {diff} of {rows} = {100.0 * diff / rows:.3f} %")


if __name__ == "__main__":
    main()
