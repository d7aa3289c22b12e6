"""Timing and resources of the elastic-net path kernel ``k_encd`` behind ``analysis.tree_prune``
(profiles/tree_prune_timing.txt, profiles/tree_prune_resources.txt).

    python tools/tree_prune_profile.py [--out profiles] [--variants encd_t64,encd_nopre]
    python tools/tree_prune_profile.py --resources          # the compiler's resource report only (no GPU)

Problem: the train split (periods 0..239) of the bench panel 600 x 3000 x 46 from ``generate_panel_fast``,
the 81 depth-4 median-split trees on the characteristics 0, 1, 2 (``k_qtree_port``), their 1555 distinct
nodes as the assets (``node_returns``, ``mv_moments``), the default 9 x 16 grid of ``prune_trees`` with
``max_assets = 40`` and ``max_sweeps = 2000``.

Measured: the device time of every launch (events around it, recorded by the launcher) and their sum,
warm, the run with the median sum of ``--repeats``; sweeps and coordinate updates per computed point and
updates per second; the same for other ``sweeps_per_launch``; the yardstick ``en_paths_numpy`` on this
machine's host for one path of the problem (the one with the median number of updates), scaled to the
grid by the updates; side builds of the extension (``engine.build --variant NAME k_encd.hip=...``, each in
a child process with ``DLAP_NATIVE=NAME``) on the same problem, whose bits have to equal the default's."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_ASSETS, MAX_SWEEPS = 40, 2000


def resources(extra=()):
    """One line per instantiation of k_encd from the compiler's resource report."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", *extra,
                            f"-I{ROOT}/csrc", "-Rpass-analysis=kernel-resource-usage", "-c", f"{ROOT}/csrc/k_encd.hip", "-o",
                            os.path.join(tmp, "k_encd.o")], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-2000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:.*?(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = m.group(2)
    out = [f"  k_encd<EPT, PRE>   VGPRs  AGPRs  SGPRs  scratch B/lane  VGPR spills  SGPR spills  waves/SIMD  static LDS   ({' '.join(extra) or 'production flags'})"]
    for c in rows:
        m = re.search(r"k_encdILi(\d+)ELb([01])EE", c["name"])
        if not m:
            continue
        out.append(f"  <{int(m.group(1)):2d}, {m.group(2)}>            {c['VGPRs']:>3s}    {c['AGPRs']:>3s}    {c['TotalSGPRs']:>3s}       {c['ScratchSize']:>3s}"
                   f"            {c['VGPRs Spill']:>3s}          {c['SGPRs Spill']:>3s}          {c['Occupancy']:>2s}       {c['LDS Size']} B")
    if any(c.get("ScratchSize") != "0" for c in rows):
        out.append("  SCRATCH IN USE")
    return out


def resource_report():
    return ["Kernel resources of csrc/k_encd.hip (gfx950, -O3 -ffp-contract=off; hipcc -Rpass-analysis=kernel-resource-usage).",
            "EPT = row elements a thread holds in registers (the launcher picks the smallest power of two >= n / threads),",
            "PRE = 1: the hinted next row is requested ahead; <1, 0> streams its row (n / threads > 32 or ENCD_PREFETCH = 0).",
            "LDS is dynamic: (3 n + EPT threads) 8 B + 4 n B + 32 B per wave = 60,052 B at n = 1555, 147,584 B at n = 4096.",
            "No scratch, no spills, no atomics in any instantiation.", "",
            "256 threads (production):", *resources(), "", "64 threads (-DENCD_THREADS=64):", *resources(("-DENCD_THREADS=64",))]


def build_problem(T, N, F, train_to):
    """(S [1][n][n], b, l1s, l2) of the profiling problem, and a line that describes it."""
    import numpy as np
    import torch
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
    from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN
    ret, feats, mask, mac = generate_panel_fast(T, N, F, 8, seed=0, device="cuda")
    s = slice(0, train_to)
    mac = (mac - mac[s].mean(0)) / (mac[s].std(0, unbiased=False) + 1e-8)
    batch = {"returns": ret[s].contiguous(), "individual_features": feats[s].contiguous(), "mask": mask[s].contiguous(),
             "macro_features": mac[s].contiguous()}
    trees, splits = ts.all_trees((0, 1, 2), 4), (2, 2, 2, 2)
    eng = GANEngine(AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4])).spec, 1, max_epochs=4)
    eng.set_data(batch)
    torch.cuda.synchronize()
    r = eng.eng.tree_sorted_portfolios(0, [list(t) for t in trees], list(splits))
    eng.eng.sync()
    cnt, sums = np.asarray(r["count"]), np.asarray(r["sum"])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, sums[..., 0] / cnt, np.nan)
    del eng
    R, un = tp.node_returns({"returns": mean, "trees": trees, "splits": splits})
    mu, S = tp.mv_moments(R)
    g = tp.prune_grid(mu, S)
    line = (f"bench panel {T} x {N} x {F} (generate_panel_fast), train split = periods 0..{train_to - 1}; {len(trees)} depth-4 trees on "
            f"characteristics 0, 1, 2 -> n = {R.shape[1]} distinct nodes; {g['b'].shape[0]} paths x {g['l1s'].shape[1]} points, "
            f"max_assets {MAX_ASSETS}, max_sweeps {MAX_SWEEPS}")
    return S[None].copy(), g["b"], g["l1s"], g["l2"], line


def measure(prob, repeats, spl=None):
    """The warm run with the median device time of ``repeats``: dict of its figures."""
    import numpy as np
    import torch
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
    dev = torch.device("cuda")
    A, b, l1s, l2 = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in prob)
    a_of = torch.zeros(b.shape[0], dtype=torch.int32, device=dev)
    runs = [tp.en_paths(A, a_of, b, l1s, l2, max_sweeps=MAX_SWEEPS, max_assets=MAX_ASSETS, sweeps_per_launch=spl)
            for _ in range(repeats + 1)][1:]
    runs.sort(key=lambda r: r["gpu_ms"])
    r = runs[len(runs) // 2]
    h = hashlib.sha256(r["theta"].tobytes() + r["sweeps"].tobytes() + r["nnz"].tobytes()).hexdigest()[:16]
    comp = r["sweeps"] > 0
    return {"gpu_ms": r["gpu_ms"], "gpu_ms_min": runs[0]["gpu_ms"], "gpu_ms_max": runs[-1]["gpu_ms"], "launches": r["launches"],
            "launch_ms": r["launch_ms"], "points": int(comp.sum()), "sweeps": int(r["sweeps"].sum()),
            "updates": int(r["path_updates"].sum()), "path_updates": [int(x) for x in r["path_updates"]],
            "path_sweeps": [int(x) for x in r["sweeps"].sum(axis=1)], "nnz_last": [int(x[c][-1]) for x, c in zip(r["nnz"], comp)],
            "hash": h}


def fmt(m, name):
    lm = m["launch_ms"]
    return (f"  {name:<34s} {m['gpu_ms']:9.3f} ms ({m['gpu_ms_min']:.3f} .. {m['gpu_ms_max']:.3f})   {m['launches']:3d} launches, "
            f"longest {max(lm):8.3f} ms, median {statistics.median(lm):8.3f} ms   {m['updates'] / m['gpu_ms'] / 1e3:7.3f} M updates/s")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--T", type=int, default=600)
    p.add_argument("--N", type=int, default=3000)
    p.add_argument("--F", type=int, default=46)
    p.add_argument("--train_to", type=int, default=240, help="periods of the train split")
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles"))
    p.add_argument("--variants", type=str, default="", help="side builds to compare (comma list of DLAP_NATIVE names)")
    p.add_argument("--spl", type=str, default="16,32,64,128,256,1024,32000", help="other sweeps_per_launch to time")
    p.add_argument("--resources", action="store_true", help="write / print the resource report and stop (no GPU)")
    p.add_argument("--no_resources", action="store_true", help="(the timing run never compiles; accepted for symmetry with the other tools)")
    p.add_argument("--problem", type=str, default=None, help="(child) time the problem of this .npz and print JSON")
    a = p.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        rl = resource_report()
        with open(os.path.join(a.out, "tree_prune_resources.txt"), "w") as fh:
            fh.write("\n".join(rl) + "\n")
        print("\n".join(rl))
        return
    import numpy as np
    if a.problem:                                  # a child with DLAP_NATIVE set: the default launch size only
        from deeplearninginassetpricing_paperreplication_amd.ops import native
        nat = native.load(required=True)
        z = np.load(a.problem)
        m = measure((z["A"], z["b"], z["l1s"], z["l2"]), a.repeats)
        m.update(threads=nat.encd_threads(), prefetch=nat.encd_prefetch())
        print("JSON " + json.dumps(m), flush=True)
        return
    if a.repeats < 7:
        raise SystemExit("at least 7 repeats")
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    A, b, l1s, l2, what = build_problem(a.T, a.N, a.F, a.train_to)
    prob = (A, b, l1s, l2)
    tl = ["tree_prune.en_paths (k_encd) on an MI355X: elastic-net coordinate-descent paths, fp64, the bits of en_paths_numpy",
          f"device time = events around every launch, summed; warm, the run with the median sum of {a.repeats} (min .. max of the sums)",
          "  python tools/tree_prune_profile.py --variants encd_t64,encd_nopre", "", what, ""]

    def say(line=""):
        print(line, flush=True)
        tl.append(line)
    for line in tl:
        print(line, flush=True)
    dflt = int(nat.ENCD_DEFAULT_SWEEPS_PER_LAUNCH)
    base = measure(prob, a.repeats)
    say(f"production build: {nat.encd_threads()} threads, next-row prefetch {'on' if nat.encd_prefetch() else 'off'}, "
        f"sweeps_per_launch {dflt} (the default)")
    say(fmt(base, f"sweeps_per_launch {dflt}"))
    say("  per launch [ms]: " + " ".join(f"{x:.3f}" for x in base["launch_ms"]))
    say(f"  {base['points']} computed points of {b.shape[0] * l1s.shape[1]}: {base['sweeps']} sweeps, {base['updates']} updates = "
        f"{base['sweeps'] / base['points']:.1f} sweeps and {base['updates'] / base['points']:.1f} updates per point, "
        f"{base['updates'] / base['sweeps']:.2f} updates per sweep (a sweep costs updates + 1 scans of n)")
    say("  per path: sweeps " + " ".join(str(x) for x in base["path_sweeps"]) + "   updates " + " ".join(str(x) for x in base["path_updates"])
        + "   nnz at the last computed point " + " ".join(str(x) for x in base["nnz_last"]))
    say()
    say("other sweeps_per_launch (same build; every run gives the same bits):")
    for spl in [int(x) for x in a.spl.split(",") if x.strip()]:
        if spl == dflt:
            continue
        m = measure(prob, a.repeats, spl)
        say(fmt(m, f"sweeps_per_launch {spl}") + ("" if m["hash"] == base["hash"] else "   BITS DIFFER"))
    say()
    # the yardstick: the numpy definition on this machine's host, one path, scaled by the updates
    order = sorted(range(b.shape[0]), key=lambda q: base["path_updates"][q])
    q = order[len(order) // 2]
    t0 = time.perf_counter()
    ref = tp.en_paths_numpy(A, [0], b[q:q + 1], l1s[q:q + 1], l2[q:q + 1], max_sweeps=MAX_SWEEPS, max_assets=MAX_ASSETS)
    sec = time.perf_counter() - t0
    ups = int(ref["updates"].sum())
    scans = ups + int(ref["sweeps"].sum())
    est = sec * (base["updates"] + base["sweeps"]) / scans
    say(f"yardstick en_paths_numpy on this host ({os.cpu_count()} CPUs, numpy {np.__version__}), path {q} only (the median by updates): "
        f"{sec:.2f} s for {ups} updates / {scans} scans = {1e6 * sec / scans:.1f} us per scan")
    say(f"  scaled by the scans to the {b.shape[0]} paths: {est:.1f} s (not run in full)  ->  kernel {est * 1e3 / base['gpu_ms']:.0f} x")
    say(f"  this path alone on the GPU would still take the longest launches' time: the paths run side by side, one workgroup each, so")
    say(f"  the device time is the slowest path's, {max(base['path_updates'])} updates: {1e3 * base['gpu_ms'] / max(base['path_updates']):.2f} us per update of one path")
    say()
    if a.variants:
        say("side builds, same problem, each in a process of its own (DLAP_NATIVE=NAME), default sweeps_per_launch:")
        with tempfile.TemporaryDirectory() as tmp:
            f = os.path.join(tmp, "problem.npz")
            np.savez(f, A=A, b=b, l1s=l1s, l2=l2)
            for v in [x.strip() for x in a.variants.split(",") if x.strip()]:
                env = dict(os.environ, DLAP_NATIVE=v, DLAP_AUTOBUILD="0")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--problem", f, "--repeats", str(a.repeats)],
                                   env=env, capture_output=True, text=True, timeout=600)
                js = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
                if r.returncode != 0 or not js:
                    say(f"  {v}: failed ({r.returncode}) {r.stderr[-300:]}")
                    continue
                m = json.loads(js[-1][5:])
                say(fmt(m, f"{v}: {m['threads']} threads, prefetch {'on' if m['prefetch'] else 'off'}")
                    + f"   {m['gpu_ms'] / base['gpu_ms']:.3f} x the production build" + ("" if m["hash"] == base["hash"] else "   BITS DIFFER"))
        say()
    with open(os.path.join(a.out, "tree_prune_timing.txt"), "w") as fh:
        fh.write("\n".join(tl) + "\n")


if __name__ == "__main__":
    main()
