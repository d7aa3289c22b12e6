"""Timing, resources and accuracy of the tree-weight kernel ``k_qtree_weight`` behind
``tree_sorts.tree_weights`` / ``tree_prune.pruned_weights`` (profiles/tree_weights_timing.txt,
profiles/tree_weights_resources.txt, profiles/tree_weights_accuracy.txt).

    python tools/tree_weights_profile.py [--out profiles] [--variants qtw_reread,qtw_seg128,qtw_seg512]
    python tools/tree_weights_profile.py --resources          # the compiler's resource report only (no GPU)

Workload: the bench panel 600 x 3000 x 46 from ``generate_panel_fast`` in its three splits (240 / 60 / 300
periods), the 81 depth-4 median-split trees on the characteristics 0, 1, 2, bf16 and fp32 panels, with (a)
the coefficients of the pruned SDF that ``prune_trees`` selects on these sorts (sparse) and (b) a dense
random table over all 81 x 31 nodes.

Measured: the device time of a call (events around the launch, ``gpu_ms`` of ``Engine.tree_weights``), warm,
the median and the minimum of ``--repeats``; next to it ``k_qtree_port`` on the same trees and split in the
same process (the yardstick: its assign sweep does the same walk plus the selects and the sums), with its
own spread (median - min) / min; ``tree_weights_numpy`` on this machine's host; a torch route that lives in
this file only; other trees-per-pass values; side builds of the extension, each in a child process with
``DLAP_NATIVE=NAME``, whose bits have to equal the default's::

    python -m deeplearninginassetpricing_paperreplication_amd.engine.build --variant qtw_reread \
        k_qtree_weight.hip=-ffp-contract=off,-DQTREE_WEIGHT_REREAD=1 $OTHER
    python -m deeplearninginassetpricing_paperreplication_amd.engine.build --variant qtw_seg128 \
        k_qtree_weight.hip=-ffp-contract=off,-DQTREE_WEIGHT_SEG=128 engine.cpp=-DQTREE_WEIGHT_SEG=128 $OTHER

(``qtw_seg512`` likewise; ``OTHER="k_encd.hip=-ffp-contract=off k_tbwd.hip=-mllvm,-amdgpu-mfma-vgpr-form"``, the production
flags of the other files: a variant's flags replace ``FILE_FLAGS``). The accuracy record counts the cells with the oracle's bits on the panels of
tests/test_tree_weights_gpu.py and states the self-check of the pruned weights on the bench panel."""
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

SPLIT_T = (("train", 0, 240), ("valid", 240, 300), ("test", 300, 600))
CHARS, DEPTH = (0, 1, 2), 4


# ---- resources (no GPU) ------------------------------------------------------------------------------
def resources(extra=()):
    """(lines, facts) of one compile of k_qtree_weight.hip: a row per instantiation from the compiler's resource
    report and the instruction counts of the file's device code; ``facts`` holds what the summary is derived from."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", *extra,
                            f"-I{ROOT}/csrc", "-Rpass-analysis=kernel-resource-usage", "-save-temps=obj", "-c",
                            f"{ROOT}/csrc/k_qtree_weight.hip", "-o", os.path.join(tmp, "k.o")], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        asm = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f]
        text = open(os.path.join(tmp, asm[0])).read() if asm else ""
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
    out = [f"  k_qtree_weight<F32, D>   VGPRs  AGPRs  SGPRs  scratch B/lane  VGPR spills  SGPR spills  waves/SIMD  static LDS   "
           f"({' '.join(extra) or 'production flags'})"]
    inst = []
    for c in rows:
        m = re.search(r"k_qtree_weightILb([01])ELi(\d)EE", c["name"])
        if m:
            inst.append((int(m.group(2)), c))
            out.append(f"  <{m.group(1)}, {m.group(2)}>                   {c['VGPRs']:>3s}    {c['AGPRs']:>3s}    {c['TotalSGPRs']:>3s}       "
                       f"{c['ScratchSize']:>3s}            {c['VGPRs Spill']:>3s}          {c['SGPRs Spill']:>3s}          {c['Occupancy']:>2s}       "
                       f"{c['LDS Size']} B")
    n = {k: len(re.findall(r"^\s+" + k, text, re.M)) for k in ("v_add_f64", "v_fma_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64",
                                                                "v_mul_f64", "global_atomic", "ds_add", "ds_cmpst", "buffer_atomic", "flat_atomic",
                                                                "scratch_")} if text else {}
    if n:
        out.append("  instructions in the file: " + "  ".join(f"{k} {v}" for k, v in n.items()))
    facts = {"instantiations": len(inst), "scratch": max((int(c["ScratchSize"]) for _, c in inst), default=-1),
             "vgpr_spills": max((int(c["VGPRs Spill"]) for _, c in inst), default=-1),
             "sgpr_spills": max((int(c["SGPRs Spill"]) for _, c in inst), default=-1),
             "vgprs": sorted({int(c["VGPRs"]) for _, c in inst}), "chain_adds": sum(2 * (d + 1) for d, _ in inst), "counts": n}
    return out, facts


def derived(facts):
    """The summary lines of one compile, every statement computed from the parsed report and counts."""
    n = facts["counts"]
    out = [f"  {facts['instantiations']} instantiations; VGPRs {facts['vgprs'][0]} .. {facts['vgprs'][-1]}; scratch at most {facts['scratch']} B/lane"
           + (" (none)" if facts["scratch"] == 0 else "  SCRATCH IN USE") + f"; VGPR spills at most {facts['vgpr_spills']}; SGPR spills at most "
           f"{facts['sgpr_spills']}" + (" (to VGPR lanes, not to memory: scratch is 0)" if facts["sgpr_spills"] and facts["scratch"] == 0 else "")]
    if n:
        atom = sum(v for k, v in n.items() if "atomic" in k or k in ("ds_add", "ds_cmpst"))
        out.append(f"  atomic instructions: {atom}; scratch instructions: {n['scratch_']}")
        div = n["v_div_fixup_f64"]
        out.append(f"  fp64 divisions (v_div_fixup_f64): {div}" + (f", v_fma_f64 per division {n['v_fma_f64'] / div:g}, v_mul_f64 per division "
                                                                 f"{n['v_mul_f64'] / div:g}" if div else ""))
        ok = n["v_add_f64"] == facts["chain_adds"] and div == facts["instantiations"]
        out.append(f"  v_add_f64 {n['v_add_f64']}, the acc chains of two trees walked side by side need sum over the instantiations of 2 (D + 1) = "
                   f"{facts['chain_adds']}: " + ("every fp64 addition is a plain v_add_f64 and the only multiply-adds are those of the one division "
                                                 "per instantiation (the staged table entry coef / count)" if ok else "COUNTS DO NOT MATCH: READ THE ASSEMBLY"))
    return out


def resource_report():
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)                      # (host functions only: no GPU is needed)
    lay = ts.tree_layout((2,) * DEPTH)
    tpp, seg = int(nat.QTREE_WEIGHT_DEFAULT_TPP), int(nat.QTREE_WEIGHT_SEG)
    work = nat.qtree_weight_lds_bytes(tpp, lay["nodes"], lay["breaks"], len(CHARS))
    most = nat.qtree_weight_lds_bytes(int(nat.QTREE_WEIGHT_MAX_TPP), 2 * ts.MAX_LEAVES, ts.MAX_LEAVES, int(nat.QTREE_WEIGHT_MAX_KEYS))
    prod, pf = resources()
    rer, rf = resources(("-DQTREE_WEIGHT_REREAD=1",))
    return ["Kernel resources of csrc/k_qtree_weight.hip (gfx950, -O3 -ffp-contract=off; hipcc -Rpass-analysis=kernel-resource-usage).",
            "F32 = 1: fp32 panel, 0: bf16 panel; D = levels of the trees (the level loop is unrolled over it).",
            f"LDS is dynamic (qtree_weight_lds_bytes): the fp64 table coef / count, the staged keys ({seg} rows), the breakpoints and the key slots:",
            f"{work:,} B for the profiled workload ({tpp} trees per pass, depth {DEPTH}: {lay['nodes']} nodes, {lay['breaks']} breakpoints, {len(CHARS)} keys); "
            f"an upper bound over all supported calls is {most:,} B ({nat.QTREE_WEIGHT_MAX_TPP} trees per pass, {2 * ts.MAX_LEAVES} nodes, "
            f"{nat.QTREE_WEIGHT_MAX_KEYS} keys).", "",
            f"{seg} rows per segment (production):", *prod, *derived(pf), "",
            "keys re-read from the panel (-DQTREE_WEIGHT_REREAD=1):", *rer, *derived(rf)]


# ---- the workload ------------------------------------------------------------------------------------
def build_panel(T, N, F):
    import torch
    from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
    ret, feats, mask, mac = generate_panel_fast(T, N, F, 8, seed=0, device="cuda")
    tr = slice(0, SPLIT_T[0][2])
    mac = (mac - mac[tr].mean(0)) / (mac[tr].std(0, unbiased=False) + 1e-8)
    out = {}
    for s, a, b in SPLIT_T:
        a, b = min(a, T), min(b, T)
        out[s] = {"returns": ret[a:b].contiguous(), "individual_features": feats[a:b].contiguous(), "mask": mask[a:b].contiguous(),
                  "macro_features": mac[a:b].contiguous()}
    torch.cuda.synchronize()
    return out


def make_engine(batch, precision):
    import torch
    from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN
    F = batch["individual_features"].shape[2]
    eng = GANEngine(AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4])).spec, 1, max_epochs=4, precision=precision)
    eng.set_data(batch)
    torch.cuda.synchronize()
    return eng


def med_min(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[0]


def time_sort(eng, trees, splits, repeats):
    import numpy as np
    runs = []
    for _ in range(repeats + 1):
        r = eng.eng.tree_sorted_portfolios(0, [list(t) for t in trees], list(splits))
        runs.append(float(r["gpu_ms"]))
    eng.eng.sync()
    cnt, sums = np.asarray(r["count"]), np.asarray(r["sum"])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, sums[..., 0] / cnt, np.nan)
    res = {"returns": mean, "count": cnt, "breaks": np.asarray(r["breaks"]), "trees": [tuple(t) for t in trees], "splits": tuple(splits),
           "names": [">".join(map(str, t)) for t in trees]}
    return res, med_min(runs[1:])


def time_weights(eng, batch, res, coef, repeats, tpp=0):
    """(w numpy, (median, min) ms, result dict) of ``repeats`` warm calls."""
    import torch
    T, N = batch["mask"].shape
    w = torch.zeros((T, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats + 1):
        r = eng.eng.tree_weights(0, [list(t) for t in res["trees"]], list(res["splits"]), res["breaks"], res["count"], coef, 0, 0,
                                 w.data_ptr(), 0, tpp)
        runs.append(float(r["gpu_ms"]))
    eng.eng.sync()
    return w.cpu().numpy(), med_min(runs[1:]), r


def held_keys(batch, precision):
    import torch
    f = batch["individual_features"]
    return (f.to(torch.bfloat16).to(f.dtype) if precision == "bf16" else f)


def torch_weights(batch, precision, res, coef, repeats):
    """The same walk in torch ops on the device (this tool's comparison only): (w, (median, min) ms)."""
    import numpy as np
    import torch
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    lay = ts.tree_layout(res["splits"])
    qs, D, off, boff = lay["splits"], lay["depth"], lay["level_offsets"], lay["break_offsets"]
    mask = batch["mask"].bool()
    t_of = torch.nonzero(mask)[:, 0]
    keys = held_keys(batch, precision)[mask]                                   # [R][F]
    brk = torch.from_numpy(res["breaks"]).cuda()
    cnt = torch.from_numpy(res["count"]).cuda().to(torch.float64)
    cf = torch.from_numpy(np.ascontiguousarray(coef)).cuda()
    act = [(p, max(l for l in range(D + 1) if np.any(coef[p, off[l]:off[l + 1]] != 0))) for p in range(coef.shape[0]) if np.any(coef[p] != 0)]
    zero = torch.zeros((), dtype=torch.float64, device="cuda")

    def once():
        acc = torch.zeros(t_of.shape[0], dtype=torch.float64, device="cuda")
        for p, depth in act:
            node = torch.zeros_like(t_of)
            for l in range(depth + 1):
                if l >= 1:
                    Q = qs[l - 1]
                    k = keys[:, res["trees"][p][l - 1]] + 0.0
                    base = boff[l - 1] + node * (Q - 1)
                    q = torch.zeros_like(node)
                    for d in range(Q - 1):
                        q = q + (k > brk[t_of, p, base + d]).long()
                    node = node * Q + q
                c = cf[p, off[l] + node]
                acc = acc + torch.where(c != 0, c / cnt[t_of, p, off[l] + node], zero)
        return acc
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats + 1)]
    for a, b in ev:
        a.record()
        acc = once()
        b.record()
    torch.cuda.synchronize()
    w = torch.zeros(mask.shape, dtype=torch.float32, device="cuda")
    w[mask] = acc.to(torch.float32)
    return w.cpu().numpy(), med_min([a.elapsed_time(b) for a, b in ev[1:]])


def same_bits(a, b, mask):
    import numpy as np
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return int((a[mask] == b[mask]).sum()), int(mask.sum())


def whash(ws):
    return hashlib.sha256(b"".join(w.tobytes() for w in ws)).hexdigest()[:16]


def reading(base, tpps, variants, seg, tpp0):
    """The closing lines: every alternative against the production call (test split, dense coef, bf16), a ratio
    inside the production call's own spread reported as no difference. ``base`` = (median, min) ms, ``tpps`` =
    {trees_per_pass: (median, min)}, ``variants`` = {name: (rows per segment, (median, min))}; ``seg`` and ``tpp0``
    the production build's rows per segment and default trees per pass."""
    bm, bn = base
    spread = (bm - bn) / bn
    out = [f"reading (test split, dense coef, bf16): production ({seg} rows per segment, keys staged in LDS, {tpp0} trees per pass) "
           f"{bm:.3f} ms, its own spread (median - min) / min = {100 * spread:.1f} %"]
    faster = []
    for tpp, (m, _) in sorted(tpps.items()):
        out.append(f"  trees_per_pass {tpp}: {ratio(m, bm, spread)}")
        if m / bm < 1.0 - spread:
            faster.append(f"trees_per_pass {tpp}")
    for v, (vs, (m, _)) in variants.items():
        out.append(f"  {v} ({vs} rows per segment): {ratio(m, bm, spread)}")
        if m / bm < 1.0 - spread:
            faster.append(v)
    out.append("  faster than the production call beyond its spread: " + (", ".join(faster) if faster else "none"))
    return out


def ratio(x, y, spread):
    """``x / y`` as text; inside the yardstick's own spread it is reported as no difference."""
    r = x / y
    return f"{r:.3f} x" + (" (no difference: inside the yardstick's spread)" if abs(r - 1.0) <= spread else "")


# ---- the panels of the GPU tests: cells with the oracle's bits ------------------------------------------
def test_panel_agreement():
    import itertools
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weight_cases as wc
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    lines = []
    cases = {"A": [(2, 2, 2), (2, 2, 2, 2, 2), (3, 3, 4), (16, 2), (6, 6)], "B": [(2, 2, 2, 2), (3, 3, 4), (2, 16), (5, 5)],
             "W": [(2, 2, 2), (3, 3, 4)]}
    for name, splits_list in cases.items():
        b, extra = wc.gpu_panel(name)
        mask = b["mask"].numpy()
        for precision in ("bf16", "fp32"):
            eng = make_engine(b, precision)
            ek = torch.as_tensor(extra).cuda().contiguous() if extra is not None else None
            E = 0 if ek is None else ek.shape[0]
            keys = wc.engine_keys(name, precision)
            eq32 = eq64 = tot = calls = 0
            for splits in splits_list:
                D = len(splits)
                if name == "A":
                    trees = wc.gpu_trees(wc.KEYS_A, D, 10)
                elif name == "B":
                    trees = list(dict.fromkeys([(5,) * D] + wc.gpu_trees(wc.KEYS_B, D, 6) + list(itertools.product((1, 5), repeat=D))[:8]
                                               + list(itertools.product((6, 2), repeat=D))[:4]))
                else:
                    trees = [(0, 129, 64), (128, 64, 0), (77, 77, 77), (129, 1, 128)]
                r = eng.eng.tree_sorted_portfolios(0, [list(t) for t in trees], list(splits), ek.data_ptr() if E else 0, E, 0, 0)
                brk, cnt = np.asarray(r["breaks"]), np.asarray(r["count"])
                NN = cnt.shape[2]
                for coef in (wc.dense_coef(len(trees), NN, 21, decades=3), wc.sparse_coef(len(trees), splits)):
                    for tpp in (0, 1, 3):
                        w = torch.zeros(mask.shape, dtype=torch.float32, device="cuda")
                        a = torch.zeros(mask.shape, dtype=torch.float64, device="cuda")
                        eng.eng.tree_weights(0, [list(t) for t in trees], list(splits), brk, cnt, coef, ek.data_ptr() if E else 0, E,
                                             w.data_ptr(), a.data_ptr(), tpp)
                        eng.eng.sync()
                        want = ts.tree_weights_numpy(keys, trees, mask, splits, brk, cnt, coef, dtype=np.float64)
                        eq32 += int((wc.bits32(w.cpu().numpy())[mask] == wc.bits32(want.astype(np.float32))[mask]).sum())
                        eq64 += int((wc.bits64(a.cpu().numpy())[mask] == wc.bits64(want)[mask]).sum())
                        tot += int(mask.sum())
                        calls += 1
            lines.append(f"  panel {name} {precision}: {calls} calls (dense and sparse coef, trees_per_pass default / 1 / 3, {len(splits_list)} splits): "
                         f"w {eq32} of {tot} cells with the oracle's bits, acc {eq64} of {tot}")
            del eng
    return lines


# ---- a child with DLAP_NATIVE set: the bf16 workload of a side build --------------------------------------
def child(a):
    import numpy as np
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    z = np.load(a.child)
    batches = build_panel(a.T, a.N, a.F)
    trees, splits = ts.all_trees(CHARS, DEPTH), (2,) * DEPTH
    out = {"seg": int(nat.QTREE_WEIGHT_SEG), "ms": {}, "ws": []}
    ws = []
    for s, _, _ in SPLIT_T:
        eng = make_engine(batches[s], "bf16")
        res, _ = time_sort(eng, trees, splits, 1)
        for kind in ("sparse", "dense"):
            w, mm, _ = time_weights(eng, batches[s], res, z[kind], a.repeats)
            out["ms"][f"{s}/{kind}"] = mm
            ws.append(w)
        del eng
    out["hash"] = whash(ws)
    print("JSON " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--T", type=int, default=600)
    p.add_argument("--N", type=int, default=3000)
    p.add_argument("--F", type=int, default=46)
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles"))
    p.add_argument("--variants", type=str, default="", help="side builds to compare (comma list of DLAP_NATIVE names)")
    p.add_argument("--tpp", type=str, default="1,2,4,8,32", help="other trees_per_pass to time")
    p.add_argument("--resources", action="store_true", help="write / print the resource report and stop (no GPU)")
    p.add_argument("--no_numpy", action="store_true", help="skip the host yardstick (it takes tens of seconds)")
    p.add_argument("--child", type=str, default=None, help="(child) time the coefficient tables of this .npz and print JSON")
    a = p.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        rl = resource_report()
        with open(os.path.join(a.out, "tree_weights_resources.txt"), "w") as fh:
            fh.write("\n".join(rl) + "\n")
        print("\n".join(rl))
        return
    if a.child:
        return child(a)
    if a.repeats < 7:
        raise SystemExit("at least 7 repeats")
    import numpy as np
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    trees, splits = ts.all_trees(CHARS, DEPTH), (2,) * DEPTH
    NN = ts.tree_layout(splits)["nodes"]
    batches = build_panel(a.T, a.N, a.F)
    rows = {s: int(b["mask"].sum()) for s, b in batches.items()}
    tl = ["tree_sorts.tree_weights (k_qtree_weight) on an MI355X: stock-level weights of a combination of tree nodes, the bits of tree_weights_numpy",
          f"device time = events around the launch; warm, median (min) of {a.repeats} calls",
          "  python tools/tree_weights_profile.py --variants qtw_reread,qtw_seg128,qtw_seg512", "",
          f"bench panel {a.T} x {a.N} x {a.F} (generate_panel_fast), splits " + ", ".join(f"{s} {b - x} periods / {rows[s]} rows" for s, x, b in SPLIT_T)
          + f"; {len(trees)} depth-{DEPTH} median-split trees on characteristics {', '.join(map(str, CHARS))} ({NN} nodes each)",
          f"production build: {nat.QTREE_WEIGHT_SEG} rows per segment (one lane per row), keys staged in LDS, "
          f"{nat.QTREE_WEIGHT_DEFAULT_TPP} trees per pass (the default)", ""]
    al = ["Accuracy of tree_sorts.tree_weights on the GPU (k_qtree_weight) against tree_weights_numpy: bitwise, no tolerance.", ""]

    def say(line=""):
        print(line, flush=True)
        tl.append(line)
    for line in tl:
        print(line, flush=True)
    rng = np.random.default_rng(7)
    dense = rng.standard_normal((len(trees), NN))
    keep = {}
    for precision in ("bf16", "fp32"):
        engs = {s: make_engine(batches[s], precision) for s, _, _ in SPLIT_T}
        by_split, sort_ms = {}, {}
        for s in engs:
            by_split[s], sort_ms[s] = time_sort(engs[s], trees, splits, a.repeats)
        pr = tp.prune_trees(by_split, device="cuda")
        sparse = tp.node_coefficients(pr, by_split["train"])
        say(f"{precision} panel; pruned selection: {len(pr['nodes'])} nodes on {int((sparse != 0).any(axis=1).sum())} trees "
            f"(l0 {pr['l0']:g}, l2 {pr['l2_rel']:g}, l1 {pr['l1']:.3e}), deepest level {max(n[3] for n in pr['nodes'])}")
        say(f"  {'split':6s} {'k_qtree_port (yardstick)':>34s} {'(a) pruned, sparse coef':>34s} {'(b) dense coef, 81 x 31':>34s}")
        pw, check = {}, 0.0
        for s in engs:
            sm, sn = sort_ms[s]
            spread = (sm - sn) / sn
            wa, (am, an), ra = time_weights(engs[s], batches[s], by_split[s], sparse, a.repeats)
            wb, (bm, bn), rb = time_weights(engs[s], batches[s], by_split[s], dense, a.repeats)
            pw[s] = wa
            keep[(precision, s)] = (by_split[s], wa, wb)
            say(f"  {s:6s} {sm:9.3f} ms ({sn:.3f}), spread {100 * spread:4.1f} %   {am:9.3f} ms ({an:.3f}) = {ratio(am, sm, spread)}   "
                f"{bm:9.3f} ms ({bn:.3f}) = {ratio(bm, sm, spread)}")
            say(f"         (a) {ra['active_trees']} active trees, {ra['passes']} pass(es), {ra['keys']} keys; (b) {rb['active_trees']} trees, "
                f"{rb['passes']} passes; {rb['segments']} segments; (b) {1e-6 * rows[s] * len(trees) * DEPTH / bm:.1f} G tree steps/s")
        pm = tp.pruned_metrics(pr, by_split, pw, {s: {k: v.cpu() for k, v in b.items()} for s, b in batches.items()})
        say(f"  self-check max |sum_i w R - R_split . theta| over the {a.T} periods: {pm['self_check']:.3e}; Sharpe from w (train / valid / test) "
            f"{pm['train_sharpe']:.4f} / {pm['valid_sharpe']:.4f} / {pm['test_sharpe']:.4f}, from R . theta {pr['train_sharpe']:.4f} / "
            f"{pr['valid_sharpe']:.4f} / {pr['test_sharpe']:.4f}")
        al.append(f"bench panel, {precision}: largest self-check |sum_i w R - R_split . theta| of the pruned weights over all {a.T} periods: "
                  f"{pm['self_check']:.3e} (the float32 rounding of w: 2^-24 sum_i |w R| per period)")
        say()
        if precision == "bf16":
            sparse_bf16, res_test = sparse, by_split["test"]
            say("other trees_per_pass, test split, dense coef (every run gives the same bits):")
            tpp_ms = {}
            for tpp in [int(x) for x in a.tpp.split(",") if x.strip()] + [0]:
                w, (m, n), r = time_weights(engs["test"], batches["test"], res_test, dense, a.repeats, tpp)
                if tpp:
                    tpp_ms[tpp] = (m, n)
                else:
                    base_ms = (m, n)
                say(f"  trees_per_pass {tpp or nat.QTREE_WEIGHT_DEFAULT_TPP:3d}{' (default)' if not tpp else '':10s} {m:9.3f} ms ({n:.3f})   {r['passes']:3d} passes"
                    + ("" if w.tobytes() == keep[("bf16", "test")][2].tobytes() else "   BITS DIFFER"))
            say()
        del engs
    def flush_files():
        with open(os.path.join(a.out, "tree_weights_timing.txt"), "w") as fh:
            fh.write("\n".join(tl) + "\n")
        with open(os.path.join(a.out, "tree_weights_accuracy.txt"), "w") as fh:
            fh.write("\n".join(al) + "\n")
    flush_files()
    # the torch route and the host yardstick, test split
    mask = batches["test"]["mask"].cpu().numpy().astype(bool)
    for precision in ("bf16", "fp32"):
        res, wa, wb = keep[(precision, "test")]
        sp_coef = sparse_bf16 if precision == "bf16" else sparse
        for kind, coef, wk in (("sparse", sp_coef, wa), ("dense", dense, wb)):
            wt, (m, n) = torch_weights(batches["test"], precision, res, coef, a.repeats)
            eq, tot = same_bits(wt, wk, mask)
            say(f"torch route (this tool only), test split, {precision}, {kind}: {m:9.3f} ms ({n:.3f}); {eq} of {tot} cells with the kernel's bits")
    say()
    flush_files()
    if not a.no_numpy:
        import torch
        for precision in ("bf16", "fp32"):
            res, wa, wb = keep[(precision, "test")]
            keys = held_keys(batches["test"], precision).cpu().numpy().astype(np.float32)
            sp_coef = sparse_bf16 if precision == "bf16" else sparse
            for kind, coef, wk in (("sparse", sp_coef, wa), ("dense", dense, wb)):
                if precision == "fp32" and kind == "dense":
                    continue                                       # (the same work as bf16 dense: not repeated)
                t0 = time.perf_counter()
                wn = ts.tree_weights_numpy(keys, trees, mask, splits, res["breaks"], res["count"], coef)
                sec = time.perf_counter() - t0
                eq, tot = same_bits(wn, wk, mask)
                say(f"tree_weights_numpy on this host ({os.cpu_count()} CPUs, numpy {np.__version__}), test split, {precision}, {kind}: {sec:.2f} s; "
                    f"{eq} of {tot} cells of the kernel's w with its bits")
                al.append(f"bench panel, test split, {precision}, {kind} coef: {eq} of {tot} cells of w with the bits of tree_weights_numpy")
        say()
        flush_files()
    var_ms = {}
    if a.variants:
        say("side builds, bf16 workload, each in a process of its own (DLAP_NATIVE=NAME), default trees_per_pass; median (min) ms:")
        base_hash = whash([keep[("bf16", s)][k] for s, _, _ in SPLIT_T for k in (1, 2)])
        with tempfile.TemporaryDirectory() as tmp:
            f = os.path.join(tmp, "coef.npz")
            np.savez(f, sparse=sparse_bf16, dense=dense)
            for v in [x.strip() for x in a.variants.split(",") if x.strip()]:
                env = dict(os.environ, DLAP_NATIVE=v, DLAP_AUTOBUILD="0")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f, "--repeats", str(a.repeats), "--T", str(a.T),
                                    "--N", str(a.N), "--F", str(a.F)], env=env, capture_output=True, text=True, timeout=300)
                js = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
                if r.returncode != 0 or not js:
                    say(f"  {v}: failed ({r.returncode}) {r.stderr[-300:]}")
                    continue
                m = json.loads(js[-1][5:])
                say(f"  {v} ({m['seg']} rows per segment): " + "  ".join(f"{k} {x[0]:.3f} ({x[1]:.3f})" for k, x in m["ms"].items())
                    + ("" if m["hash"] == base_hash else "   BITS DIFFER"))
                var_ms[v] = (m["seg"], tuple(m["ms"]["test/dense"]))
        say()
    for line in reading(base_ms, tpp_ms, var_ms, int(nat.QTREE_WEIGHT_SEG), int(nat.QTREE_WEIGHT_DEFAULT_TPP)):
        say(line)
    say()
    flush_files()
    al.append("")
    al.append("panels of tests/test_tree_weights_gpu.py (the engine's own breaks / count, the oracle on the keys the engine holds):")
    al.extend(test_panel_agreement())
    print("\n".join(al), flush=True)
    flush_files()


if __name__ == "__main__":
    main()
