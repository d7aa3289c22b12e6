"""Timing, accuracy and kernel resources of the characteristic-Gram kernel (``csrc/k_xgram.hip``) and
of the IPCA row built on it: writes ``ipca_timing.txt`` and ``ipca_accuracy.txt`` into ``--out_dir``.

    python tools/ipca_profile.py [--out_dir profiles] [--variants xgram32 xgram512]

GPU only. Timing: ``Engine.characteristic_gram`` (``gpu_ms``: events around the launch on the engine
stream; median and min of the warm repeats) on the three splits (240 / 60 / 300 periods) of the
bench panel 600 x 3000 x 46 and on one 60-period split of the scaled panel (x 30000 x 512, the wide
layer-0 path), per panel precision; next to it ``k_managed`` on the same split (it streams the same
rows once: the floor) and a torch baseline on the same GPU, ``bmm(X_t', X_t)`` in fp32 on a dense
masked copy. ``--variants``: side builds of ``XGRAM_RUN`` (``engine.build --variant NAME
k_xgram.hip=-DXGRAM_RUN=n ...``), each timed in a child process with ``DLAP_NATIVE=NAME``.
Accuracy: the largest |kernel - numpy| / bound (the bound of ``tests/test_xgram_gpu.py``) per panel
and the end-to-end differences of the IPCA row between the engine and numpy. Resources:
``hipcc -Rpass-analysis=kernel-resource-usage`` of the kernel file."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearninginassetpricing_paperreplication_amd.analysis import benchmarks as bm  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.analysis import ipca  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine  # noqa: E402

U = 2.0 ** -24


def _med(call, repeats):
    ms = [float(call()["gpu_ms"]) for _ in range(repeats + 1)]
    return statistics.median(ms[1:]), min(ms[1:])


def _time_torch(fn, repeats):
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


def _batches(T, N, F, cuts):
    ret, feats, mask, mac = generate_panel_fast(T, N, F, 8, seed=0, device="cuda")
    mac = (mac - mac[:cuts[0]].mean(0)) / (mac[:cuts[0]].std(0, unbiased=False) + 1e-8)
    c = np.cumsum([0] + list(cuts))
    return [{"returns": ret[s0:s1].contiguous(), "individual_features": feats[s0:s1].contiguous(),
             "mask": mask[s0:s1].contiguous(), "macro_features": mac[s0:s1].contiguous()} for s0, s1 in zip(c[:-1], c[1:])]


PANELS = {"bench": (600, 3000, 46, (240, 60, 300)), "scaled": (60, 30000, 512, (60,))}


def time_panel(label, repeats, torch_too=True):
    """Timing lines of one panel, both precisions (and the torch baseline)."""
    T, N, F, cuts = PANELS[label]
    batches = _batches(T, N, F, cuts)
    names = bm.SPLITS if len(cuts) == 3 else ("split",)
    rows = [int(b["mask"].sum()) for b in batches]
    out = []
    for prec in ("bf16", "fp32"):
        eng = GANEngine(bm.default_spec(F, 8), 1, max_epochs=4, precision=prec)
        eng.set_data(*batches)
        torch.cuda.synchronize()
        e, KP, eb = eng.eng, eng.KP, 4 if prec == "fp32" else 2
        for s, name in enumerate(names):
            R = rows[s]
            by = R * KP * eb + R * 4
            md, mn = _med(lambda: e.characteristic_gram(s), repeats)
            mmd, mmn = _med(lambda: e.managed_portfolios(s), repeats)
            out.append(f"  {label:<6s} {prec}  {name:<5s}  run {int(e.xgram_run()):3d}  k_xgram gpu_ms {md:9.4f} / {mn:9.4f}   "
                       f"{2.0 * R * F * F / md / 1e9:7.2f} TF/s (2 R F^2)  {by / md / 1e6:7.1f} GB/s of {by / 1e6:8.2f} MB   "
                       f"k_managed gpu_ms {mmd:8.4f} / {mmn:8.4f}   k_xgram / k_managed {md / mmd:6.1f}")
        e.sync()
        del eng
    if torch_too:
        for s, name in enumerate(names):
            b = batches[s]
            x = (b["individual_features"].float() * b["mask"][:, :, None]).contiguous()
            md, mn = _time_torch(lambda: torch.bmm(x.transpose(1, 2), x), repeats)
            out.append(f"  {label:<6s} torch {name:<5s}  bmm(X_t', X_t) fp32 on the dense masked copy [{x.shape[0]}][{N}][{F}] "
                       f"({x.numel() * 4 / 1e6:.0f} MB)  ms {md:9.4f} / {mn:9.4f}   {2.0 * x.shape[0] * N * F * F / md / 1e9:7.2f} TF/s")
            del x
    return out


def resources():
    """Per kernel: VGPRs, AGPRs, scratch, occupancy from the compiler's remarks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "csrc", "k_xgram.hip")
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
    out = ["  kernel          VGPRs  AGPRs  scratch B/lane  VGPR spills  SGPR spills  waves/SIMD  static LDS B"]
    for c in rows:
        lab = "k_xgram fp32" if "ILb1" in c["name"] else "k_xgram bf16"
        out.append(f"  {lab:<14s} {c.get('VGPRs', -1):5d}  {c.get('AGPRs', -1):5d}  {c.get('ScratchSize', -1):14d}  "
                   f"{c.get('VGPRs Spill', -1):11d}  {c.get('SGPRs Spill', -1):11d}  {c.get('Occupancy', -1):10d}  "
                   f"{c.get('LDS Size', -1):12d}")
    return out


def gram_bound(x, m, S, ref):
    ax = np.abs(x.astype(np.float64)) * m[:, :, None]
    P = np.einsum("tna,tnb->tab", ax, ax)
    n = m.sum(1).astype(np.float64)[:, None, None]
    return (S + 2) * U * P + n * 2.0 ** -52 * P + np.spacing(np.abs(ref))


def accuracy_panel(label, periods):
    """Largest |kernel - numpy| / bound on the first ``periods`` periods of a panel's split."""
    T, N, F, cuts = PANELS[label]
    b = {k: v[:periods].contiguous() for k, v in _batches(T, N, F, cuts)[1 if len(cuts) == 3 else 0].items()}
    out = []
    for prec in ("bf16", "fp32"):
        eng = GANEngine(bm.default_spec(F, 8), 1, max_epochs=4, precision=prec)
        eng.set_data(b)
        S = int(eng.eng.xgram_run())
        f = b["individual_features"]
        x = (f.to(torch.bfloat16).float() if prec == "bf16" else f).cpu().numpy()
        r, m = b["returns"].cpu().numpy(), b["mask"].cpu().numpy()
        ref = ipca.characteristic_gram_numpy(x, r, m)
        got = eng.eng.characteristic_gram(0)
        g = np.asarray(got["gram"])
        ratio = float((np.abs(g - ref["gram"]) / gram_bound(x, m, S, ref["gram"])).max())
        assert (np.asarray(got["n"]) == ref["n"]).all() and g.tobytes() == np.ascontiguousarray(g.transpose(0, 2, 1)).tobytes()
        n = ref["n"].astype(np.float64)
        rr = float((np.abs(np.asarray(got["sum_rr"]) - ref["sum_rr"]) / (n * 2.0 ** -52 * ref["sum_rr"] + np.spacing(ref["sum_rr"]))).max())
        out.append(f"  {label:<6s} {prec}  {periods} periods x {N} x {F} ({int(m.sum())} rows), run {S}: gram largest ratio {ratio:.4f}, "
                   f"sum_rr largest ratio {rr:.4f}; n exact, gram bitwise symmetric")
        del eng
    return out


def _planted():
    T, N, F, K = 60, 200, 8, 2
    rng = np.random.default_rng(0)
    x = rng.standard_normal((T, N, F)).astype(np.float32)
    g0 = np.linalg.qr(rng.standard_normal((F, K)))[0]
    f = rng.standard_normal((T, K)) * np.array((0.08, 0.05)) + np.array((0.03, 0.01))
    r = (np.einsum("tnf,fk,tk->tn", x.astype(np.float64), g0, f) + 0.1 * rng.standard_normal((T, N))).astype(np.float32)
    mask = rng.uniform(size=(T, N)) > 0.2
    mac = np.random.default_rng(77).standard_normal((T, 8)).astype(np.float32)
    out, a = {}, 0
    for name, k in zip(bm.SPLITS, (36, 12, 12)):
        out[name] = {"individual_features": torch.from_numpy(x[a:a + k]), "returns": torch.from_numpy(r[a:a + k]),
                     "mask": torch.from_numpy(mask[a:a + k]), "macro_features": torch.from_numpy(mac[a:a + k])}
        a += k
    return out


def end_to_end(label, batches, factors):
    """Largest differences of the IPCA row, engine (per precision) against numpy on the features as
    the engine stores them, with the loadings estimated on each side."""
    out = []
    for prec in ("bf16", "fp32"):
        bl = batches
        if prec == "bf16":
            bl = {s: dict(b, individual_features=b["individual_features"].to(torch.bfloat16).float()) for s, b in batches.items()}
        cpu = ipca.ipca_benchmark({s: {k: v.cpu() for k, v in b.items()} for s, b in bl.items()}, factors=factors, device="cpu")
        gpu = ipca.ipca_benchmark(batches, factors=factors, device="cuda", precision=prec)
        line = f"  {label:<8s} {prec}  K = {gpu['K']} (numpy: {cpu['K']}), iterations {gpu['iterations']} (numpy: {cpu['iterations']})"
        if gpu["K"] == cpu["K"]:
            pj = np.abs(gpu["gamma"] @ gpu["gamma"].T - cpu["gamma"] @ cpu["gamma"].T).max()
            d = {k: max(abs(gpu[k][s] - cpu[k][s]) for s in bm.SPLITS) for k in ("sharpe", "ev", "ev_factors", "xs_r2")}
            line += f": |d Gamma Gamma'| {pj:.2e}  " + "  ".join(f"|d {k}| {v:.2e}" for k, v in d.items())
            line += f"  (test: SR {gpu['sharpe']['test']:.4f}, EV {gpu['ev']['test']:.4f}, EV factors {gpu['ev_factors']['test']:.4f})"
        out.append(line)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out_dir", type=str, default=os.path.join(ROOT, "profiles"))
    p.add_argument("--variants", type=str, nargs="*", default=[], help="side builds to time (DLAP_NATIVE names)")
    p.add_argument("--timing_rows", action="store_true", help="print the k_xgram timing lines only (used for --variants)")
    a = p.parse_args()
    if a.repeats < 7:
        raise SystemExit("at least 7 repeats")
    if a.timing_rows:
        for label in PANELS:
            print("\n".join(time_panel(label, a.repeats, torch_too=False)), flush=True)
        return
    os.makedirs(a.out_dir, exist_ok=True)
    tl = ["Engine.characteristic_gram (k_xgram) on an MI355X, next to Engine.managed_portfolios (k_managed: the same rows",
          "streamed once, the floor) and a torch baseline on the same GPU",
          f"gpu_ms = events around the launch on the engine stream, median / min of {a.repeats} warm repeats",
          "  python tools/ipca_profile.py --variants xgram32 xgram512", "",
          "bench panel 600 x 3000 x 46 (generate_panel_fast), splits train / valid / test = 240 / 60 / 300 periods, fused layer-0 path;",
          "scaled panel: one split of 60 periods x 30000 x 512, wide layer-0 path.",
          "TF/s counts the full square, 2 R F^2; the kernel computes the tile pairs a <= b only. GB/s = the stored rows once",
          "(R x KP x 2 or 4 B + R x 4 B) / gpu_ms; a workgroup re-reads its period's rows once per group of four super-tiles.", ""]
    for label in PANELS:
        tl += time_panel(label, a.repeats)
        tl.append("")
    for v in a.variants:
        env = dict(os.environ, DLAP_NATIVE=v)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing_rows", "--repeats", str(a.repeats)],
                           env=env, capture_output=True, text=True, timeout=900)
        tl.append(f"side build {v} (DLAP_NATIVE={v}):")
        tl += [ln for ln in r.stdout.splitlines() if "k_xgram" in ln] if r.returncode == 0 else [f"  (failed: {r.stderr[-300:]})"]
        tl.append("")
    tl += ["Kernel resources (gfx950, -O3; hipcc -Rpass-analysis=kernel-resource-usage). F is a run-time argument, so one",
           "kernel per precision serves F = 46, 130 and 512; LDS is dynamic: 32 x (24 x 32 + 16) B = 24.5 KB (bf16) or",
           "32 x (24 x 64 + 16) B = 48.5 KB (fp32) of row image + 272 B of tables."] + resources()
    al = ["Accuracy of Engine.characteristic_gram (k_xgram) and of the IPCA row built on it, on an MI355X",
          "  python tools/ipca_profile.py", "",
          "Largest |kernel - numpy| / bound, bound = (S + 2) 2^-24 P + n 2^-52 P + 1 ulp with P = sum_i |x_a x_b| and S = XGRAM_RUN",
          "(tests/test_xgram_gpu.py), numpy on the features as stored:"]
    al += accuracy_panel("bench", 60) + accuracy_panel("scaled", 4)
    al += ["", "IPCA row end to end: engine against numpy on the features as the engine stores them (bf16-rounded for the bf16",
           "panel), loadings estimated on each side (ALS to 1e-8); the largest difference over the three splits:"]
    al += end_to_end("planted", _planted(), (2,))
    T, N, F, cuts = PANELS["bench"]
    al += end_to_end("bench", dict(zip(bm.SPLITS, _batches(T, N, F, cuts))), (1, 2, 3))
    al += ["(planted: the panel of tests/test_ipca.py (60 x 200 x 8, K = 2, seed 0), split 36 / 12 / 12; the test's tolerance there is",
           " 4 x the change under a +- bound perturbation of the numpy Gram: see its printed figures.)"]
    for name, lines in (("ipca_timing.txt", tl), ("ipca_accuracy.txt", al)):
        with open(os.path.join(a.out_dir, name), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
