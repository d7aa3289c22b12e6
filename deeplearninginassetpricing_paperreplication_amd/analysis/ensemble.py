"""Ensemble evaluation: average the L1-normalised SDF weights of several trained models.

Behaviour of `/root/reference/src/evaluate_ensemble.py` (load each checkpoint's
``config.json`` + ``best_model_sharpe.pt``, weights per split, average, re-normalise, paper-sign
Sharpe with ddof=0; individual test Sharpe; comparison with the paper's 0.75), same CLI
(``--data_dir --checkpoint_dirs ...``) plus ``--device``.

On a GPU the weights of all checkpoints that share an architecture are produced by ONE batched
native-engine forward per split (models stacked along the engine's job axis) instead of one
PyTorch forward per model; they stay on the device, where the K11 kernel (``k_ensemble``)
averages, re-normalises and forms the portfolio series (one host transfer per split).
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from ..data.dataset import load_splits
from ..models.gan import AssetPricingGAN
from .portfolio import (PAPER_TEST_SHARPE, average_weights, ensemble_sharpes, ensemble_sharpes_device,
                        paper_metrics)
from .portfolio import sharpe_ddof0 as compute_sharpe  # noqa: F401  (reference name)

SPLITS = ("train", "valid", "test")


def load_model(checkpoint_dir: str, device: str = "cpu", which: str = "best_model_sharpe.pt"):
    """``AssetPricingGAN`` from ``config.json`` + a state_dict file (safe tensor-only load)."""
    with open(os.path.join(checkpoint_dir, "config.json")) as fh:
        config = json.load(fh)
    model = AssetPricingGAN(config)
    sd = torch.load(os.path.join(checkpoint_dir, which), map_location="cpu", weights_only=True)
    model.load_state_dict(sd)
    model.to(device).eval()
    return model, config


def get_weights_from_model(model, data: Dict, device: str = "cpu") -> np.ndarray:
    macro = data.get("macro_features")
    with torch.no_grad():
        w, _ = model.get_weights(None if macro is None else macro.to(device),
                                 data["individual_features"].to(device), data["mask"].to(device),
                                 normalized=True)
    return w.detach().cpu().numpy()


def weights_batched_gpu(models: Sequence, batches: Dict[str, Dict],
                        splits: Sequence[str] = SPLITS) -> Dict[str, torch.Tensor]:
    """L1-normalised weights of every model on every split as CUDA tensors [G, T, N] (model
    order), one batched engine forward per split for each group of models that share an
    architecture. Everything stays on the device: the engine's ``wn`` buffers are copied
    device-to-device into the stack (ordered after torch's stream with events, no host sync) and
    normalised there. ``splits``: the keys of ``batches`` to evaluate (at most three)."""
    from ..engine.runner import GANEngine
    dev = torch.device("cuda", torch.cuda.current_device())
    ts = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for split in splits:
        T, N = batches[split]["mask"].shape
        out[split] = torch.empty(len(models), T, N, dtype=torch.float32, device=dev)
    groups: Dict[object, List[int]] = {}
    for i, m in enumerate(models):
        groups.setdefault(m.spec, []).append(i)
    for spec, idx in groups.items():
        eng = GANEngine(spec, len(idx), max_epochs=4)
        eng.set_data(*[batches[split] for split in splits])
        for g, i in enumerate(idx):
            eng.set_model(g, models[i], 0)
        e = eng.eng
        e.join_from(ts)
        for s, split in enumerate(splits):
            e.forward_split(s, False, False)
            for g, i in enumerate(idx):
                e.copy_ws(g, s, "wn", out[split][i].data_ptr())
        e.join_to(ts)
        e.sync()         # the engine (and its buffers) may be freed after this group
    for split in splits:                 # per (model, period) L1 normalisation over the stocks
        m = batches[split]["mask"].to(dev).float()
        W = out[split]
        out[split] = W / (W.abs() * m[None]).sum(dim=2, keepdim=True).clamp(min=1e-8)
    return out


def evaluate_ensemble(checkpoint_dirs: Sequence[str], data_dir: str, device: str = "cpu",
                      verbose: bool = True, paper: bool = False, importance: bool = False,
                      importance_split: str = "test", importance_out: str = None,
                      importance_macro_lags: int = 0, sorted_portfolios: bool = False,
                      sort_split: str = "test", sort_quantiles: int = 10, sort_out: str = None,
                      weight_structure: bool = False, structure_split: str = "test", structure_points: int = 21,
                      structure_pairs=None, structure_out: str = None, double_sorts=None,
                      double_quantiles=(5, 5), double_mode: str = "conditional", double_out: str = None,
                      benchmarks: bool = False, benchmark_grid=(16, 4), benchmark_center: str = "mean",
                      benchmarks_out: str = None, benchmark_ffn: bool = False, beta_network: bool = False,
                      prediction_epochs: int = 64, prediction_lr: float = None, prediction_seeds=(0,),
                      prediction_out: str = None, benchmark_ipca: bool = False, ipca_factors=(1, 2, 3, 4, 5, 6),
                      ipca_intercept: bool = True, fama_macbeth: bool = False, fm_out: str = None,
                      knockout: bool = False, knockout_split: str = "test", knockout_groups=None,
                      knockout_base="zero", knockout_xs_r2: bool = False, knockout_out: str = None,
                      knockout_macro: bool = False, knockout_macro_groups=None, knockout_macro_base="zero",
                      tree_sorts=None, tree_chars=None, tree_depth: int = 3, tree_splits=2,
                      tree_out: str = None, tree_prune: bool = False, prune_max_assets: int = 40,
                      prune_grid="3x3x16", prune_out: str = None, prune_metrics: bool = False,
                      prune_weights_out: str = None) -> Dict:
    """Reference output and return value; ``paper=True`` (CLI ``--paper_metrics``) adds the
    paper's EV / XS-R² / turnover / max 1-month loss of the ensemble's SDF factor per split;
    ``importance=True`` (CLI ``--variable_importance``) adds the sensitivity ranking of the
    ensemble weight on ``importance_split`` (``analysis.importance``) under the key
    ``variable_importance`` and writes it to ``importance_out`` (JSON) when given;
    ``importance_macro_lags = L > 0`` (CLI ``--importance_macro_lags``) adds the importance of
    the macro series through the LSTM for the lags 0 .. L-1 to that ranking;
    ``sorted_portfolios=True`` (CLI ``--sorted_portfolios``) adds the quantile portfolios of
    ``sort_split`` sorted on every characteristic and on the ensemble weight, priced by the SDF
    (``analysis.sorted_portfolios``), under the key ``sorted_portfolios`` and writes them to
    ``sort_out`` (JSON) when given;
    ``weight_structure=True`` (CLI ``--weight_structure``) adds the response curves of every
    characteristic on ``structure_split`` over ``structure_points`` grid points, and the
    interaction surfaces of ``structure_pairs`` (``"all"``, a list of (a, b), or the CLI's comma
    list of ``A:B`` by name or column), under the key ``weight_structure``
    (``analysis.weight_structure``) and writes them to ``structure_out`` (JSON) when given;
    ``double_sorts`` (CLI ``--double_sorts``: a list of (A, B), or the CLI's comma list of ``A:B`` by
    name, column or ``weight``) adds the ``double_quantiles`` = (Qa, Qb) double-sorted portfolios
    of ``sort_split`` (``double_mode``: ``conditional`` or ``independent``), priced by the SDF
    (``analysis.sorted_portfolios.double_sorted_portfolios``), under the key ``double_sorts`` and
    writes them to ``double_out`` (JSON) when given;
    ``benchmarks=True`` (CLI ``--benchmarks``) adds the linear (LS) and elastic-net (EN) benchmark
    SDFs (``analysis.benchmarks``: EN over the ``benchmark_grid`` = (n1, n2) penalties, selected on
    the validation split; ``benchmark_center``: ``mean`` or ``none``) next to the ensemble in one
    table, under the key ``benchmarks``, and writes them to ``benchmarks_out`` (JSON) when given;
    ``benchmark_ffn=True`` (CLI ``--benchmark_ffn``, with ``benchmarks``) adds the FFN
    return-prediction benchmark (``analysis.prediction.ffn_benchmark``) as a row between EN and the
    ensemble (key ``benchmarks["ffn"]``, ``FFN`` in the JSON);
    ``beta_network=True`` (CLI ``--beta_network``) fits the beta network to the ensemble's SDF factor
    (``analysis.prediction.beta_network``) and prints EV / XS-R² with its loadings per split next to
    the proxy figures, under the key ``beta_network``. Both towers take the architecture of the
    first checkpoint's config and ``prediction_epochs`` / ``prediction_lr`` / ``prediction_seeds``;
    ``prediction_out`` (JSON) holds whichever of the two ran;
    ``benchmark_ipca=True`` (CLI ``--benchmark_ipca``, with ``benchmarks``) adds the IPCA benchmark
    (``analysis.ipca.ipca_benchmark``: ``ipca_factors`` candidates of ``K``, selected on the validation
    split; ``ipca_intercept``) as a row ``IPCA (K=k)`` between EN and FFN (key ``benchmarks["ipca"]``,
    ``IPCA`` in the JSON);
    ``fama_macbeth=True`` (CLI ``--fama_macbeth``) prints the Fama-MacBeth slope table of ``sort_split``
    (``analysis.ipca.fama_macbeth``), under the key ``fama_macbeth``, and writes it to ``fm_out`` (JSON)
    when given. Both use the per-period characteristic Gram: ``Engine.characteristic_gram`` with
    ``device="cuda"``, numpy otherwise;
    ``knockout=True`` (CLI ``--knockout``) adds the characteristic knock-outs of ``knockout_split``
    (``analysis.knockout.knockout_importance``: the baseline, one scenario per characteristic and one per
    entry of ``knockout_groups``, a dict or the CLI's JSON file of name -> columns or names; ``knockout_base``:
    ``zero``, ``median`` or an [F] array; ``knockout_xs_r2`` adds XS-R²) under the key ``knockout``, prints
    one table (scenario, Sharpe, d Sharpe, EV, d EV) and writes the report to ``knockout_out`` (JSON) when
    given; ``knockout_macro=True`` (CLI ``--knockout_macro``, with ``knockout``) adds one scenario per macro
    series held at ``knockout_macro_base`` (``zero``: the training mean, ``median`` or an [M] array) over the
    whole split, through the LSTM, and ``knockout_macro_groups`` (a dict or the CLI's JSON file of name ->
    series or names) one per group; the table labels them by the names the macro importance report uses;
    ``tree_sorts`` (CLI ``--tree_sorts``: a list of key sequences, or the CLI's comma list of ``A:B:C`` by
    name, column or ``weight``) and / or ``tree_chars`` with ``tree_depth`` (CLI ``--tree_chars A,B,C
    --tree_depth D``: every ordered sequence of ``D`` of these keys, the asset-pricing-tree set) add the
    tree-sorted portfolios of ``sort_split`` (``analysis.tree_sorts``; ``tree_splits``: one integer for
    every level or ``2x3x3``, at most 36 leaves and 4096 trees), priced by the SDF, under the key
    ``tree_sorts`` and write them to ``tree_out`` (JSON) when given.
    ``tree_prune=True`` (CLI ``--tree_prune``, with ``tree_sorts`` or ``tree_chars``) sorts the same trees
    on all three splits and prunes their nodes into a sparse mean-variance SDF (``analysis.tree_prune``:
    at most ``prune_max_assets`` nodes, ``prune_grid`` = ``N0xN2xN1`` penalties of ``l0 x l2 x l1``,
    selected on the validation split), printed next to the ensemble under the key ``tree_prune`` and
    written to ``prune_out`` (JSON) when given. ``prune_metrics=True`` (CLI ``--prune_metrics``, with
    ``tree_prune``) forms the stock-level weights of the pruned SDF (``tree_prune.pruned_weights``) and prints
    its EV / XS-R2 / turnover / max 1-month loss on the test split, the Sharpe ratios recomputed from the
    weights and the self-check ``max |sum_i w R - R_split . theta|``, under the key ``tree_prune_metrics`` (and
    in ``prune_out``); ``prune_weights_out`` (``.npz``) saves the three dense weights."""
    say = print if verbose else (lambda *a, **k: None)
    bar = "=" * 70
    if tree_prune and not (tree_sorts or tree_chars):
        raise ValueError("tree_prune needs tree_sorts or tree_chars (CLI: --tree_prune with --tree_sorts / --tree_chars)")
    if (prune_metrics or prune_weights_out) and not tree_prune:
        raise ValueError("prune_metrics needs tree_prune (CLI: --prune_metrics with --tree_prune)")
    say(bar); say(f"ENSEMBLE EVALUATION ({len(checkpoint_dirs)} models, averaged weights)"); say(bar); say()
    datasets = load_splits(data_dir)
    batches = {s: d.get_full_batch() for s, d in zip(SPLITS, datasets)}
    say("Loaded data:")
    for s in SPLITS:
        say(f"  {s.capitalize():6s} {batches[s]['returns'].shape[0]} periods")
    say()
    say(f"Loading {len(checkpoint_dirs)} models...")
    models = []
    for i, d in enumerate(checkpoint_dirs):
        say(f"  Model {i + 1}/{len(checkpoint_dirs)}: {os.path.basename(os.path.normpath(d))}")
        models.append(load_model(d, "cpu")[0])
    np_batches = {s: {"returns": batches[s]["returns"].numpy(), "mask": batches[s]["mask"].numpy()}
                  for s in SPLITS}
    if str(device).startswith("cuda"):
        # batched engine forward + K11 (k_ensemble) averaging on the device: the [T] ensemble
        # and [G, T] individual portfolio series are the only host transfers
        wdev = weights_batched_gpu(models, batches)
        res = ensemble_sharpes_device(wdev, np_batches)
        weights = None
        if paper:
            weights = [{s: wdev[s][i].cpu().numpy() for s in SPLITS} for i in range(len(models))]
    else:
        weights = [{s: get_weights_from_model(m, batches[s], "cpu") for s in SPLITS} for m in models]
        res = ensemble_sharpes(weights, np_batches)
    ind = res["individual_sharpes"]
    say(); say(bar); say("INDIVIDUAL MODEL RESULTS (for comparison)"); say(bar); say()
    for i, s in enumerate(ind):
        say(f"  Model {i + 1}: Test Sharpe = {s:.4f}")
    say(); say(f"  Mean of individual models: {np.mean(ind):.4f}")
    say(f"  Std of individual models:  {np.std(ind):.4f}")
    say(); say(bar); say("ENSEMBLE RESULTS (averaged weights)"); say(bar); say()
    for s in SPLITS:
        say(f"  {s.capitalize()} Sharpe: {res[s + '_sharpe']:.4f}")
    say(); say(bar); say("COMPARISON WITH PAPER"); say(bar); say()
    say(f"  Paper GAN Test Sharpe:     {PAPER_TEST_SHARPE}")
    say(f"  Our Ensemble Test Sharpe:  {res['test_sharpe']:.4f}")
    say(f"  Ratio (Our / Paper):       {res['test_sharpe'] / PAPER_TEST_SHARPE:.1%}")
    say()
    out = {"train_sharpe": res["train_sharpe"], "valid_sharpe": res["valid_sharpe"],
           "test_sharpe": res["test_sharpe"], "individual_sharpes": ind}
    if paper:
        out["paper_metrics"] = {}
        say(bar); say("PAPER METRICS OF THE ENSEMBLE SDF FACTOR (Table I / A.VI / A.VII)"); say(bar); say()
        for s in SPLITS:
            b = np_batches[s]
            avg = average_weights([w[s] for w in weights], b["mask"])
            pm = paper_metrics(avg, b["returns"], b["mask"])
            out["paper_metrics"][s] = pm
            say(f"  {s.capitalize():5s}  SR {pm['sharpe']:7.4f}  EV {pm['ev']:7.4f}  XS-R2 {pm['xs_r2']:7.4f}  "
                f"turnover {pm['turnover']:6.3f}  max 1m loss {pm['max_1m_loss_std']:5.2f} sd")
        say()
    if importance:
        from .importance import format_importance, to_json, variable_importance
        if importance_split not in SPLITS:
            raise ValueError(f"importance_split must be one of {SPLITS}")
        ds = datasets[SPLITS.index(importance_split)]
        kw = {}
        if importance_macro_lags:
            kw = dict(macro_lags=int(importance_macro_lags), macro_names=getattr(ds, "macro_names", None))
        imp = variable_importance(models, batches[importance_split], device=device,
                                  names=getattr(ds, "variable_names", None), **kw)
        out["variable_importance"] = imp
        say(bar); say(f"VARIABLE IMPORTANCE ({importance_split} split, ensemble weight)"); say(bar); say()
        for line in format_importance(imp):
            say(line)
        say()
        if importance_out:
            with open(importance_out, "w") as fh:
                json.dump(to_json(imp), fh, indent=1)
            say(f"  Saved: {importance_out}"); say()
    if sorted_portfolios:
        from . import sorted_portfolios as sp
        if sort_split not in SPLITS:
            raise ValueError(f"sort_split must be one of {SPLITS}")
        ds = datasets[SPLITS.index(sort_split)]
        b = batches[sort_split]
        if str(device).startswith("cuda"):
            wavg = average_weights(list(wdev[sort_split].cpu().numpy()), np_batches[sort_split]["mask"])
        else:
            wavg = average_weights([w[sort_split] for w in weights], np_batches[sort_split]["mask"])
        res_sp = sp.sorted_portfolios(models, b, device=device, quantiles=sort_quantiles,
                                      names=getattr(ds, "variable_names", None), weights=wavg)
        priced = sp.price_portfolios(res_sp, wavg, np_batches[sort_split]["returns"], np_batches[sort_split]["mask"])
        out["sorted_portfolios"] = {"portfolios": res_sp, "priced": priced}
        say(bar); say(f"SORTED PORTFOLIOS ({sort_split} split, {res_sp['quantiles']} buckets, equally weighted)")
        say(bar); say()
        for line in sp.format_sorted(priced):
            say(line)
        say()
        if sort_out:
            with open(sort_out, "w") as fh:
                json.dump(sp.to_json(res_sp, priced), fh, indent=1)
            say(f"  Saved: {sort_out}"); say()
    if double_sorts:
        from . import sorted_portfolios as sp
        from .weight_structure import parse_pairs
        if sort_split not in SPLITS:
            raise ValueError(f"sort_split must be one of {SPLITS}")
        if double_mode not in ("conditional", "independent"):
            raise ValueError("double_mode must be conditional or independent")
        ds = datasets[SPLITS.index(sort_split)]
        b = batches[sort_split]
        F = int(b["individual_features"].shape[2])
        names = getattr(ds, "variable_names", None)
        keyn = ([str(n) for n in names] if names is not None and len(names) == F else [str(j) for j in range(F)]) + ["weight"]
        if str(device).startswith("cuda"):
            wavg = average_weights(list(wdev[sort_split].cpu().numpy()), np_batches[sort_split]["mask"])
        else:
            wavg = average_weights([w[sort_split] for w in weights], np_batches[sort_split]["mask"])
        res_ds = sp.double_sorted_portfolios(models, b, parse_pairs(double_sorts, keyn), device=device,
                                             quantiles=sp.parse_double_quantiles(double_quantiles),
                                             conditional=double_mode == "conditional", names=names, weights=wavg)
        priced = sp.price_double_sorted(res_ds, wavg, np_batches[sort_split]["returns"], np_batches[sort_split]["mask"])
        out["double_sorts"] = {"portfolios": res_ds, "priced": priced}
        qa, qb = res_ds["quantiles"]
        say(bar); say(f"DOUBLE-SORTED PORTFOLIOS ({sort_split} split, {qa} x {qb} cells, {res_ds['mode']}, equally weighted)")
        say(bar); say()
        for line in sp.format_double_sorted(priced):
            say(line)
        say()
        if double_out:
            with open(double_out, "w") as fh:
                json.dump(sp.double_to_json(res_ds, priced), fh, indent=1)
            say(f"  Saved: {double_out}"); say()
    if tree_sorts or tree_chars:
        from . import tree_sorts as ts
        if sort_split not in SPLITS:
            raise ValueError(f"sort_split must be one of {SPLITS}")
        ds = datasets[SPLITS.index(sort_split)]
        b = batches[sort_split]
        names = getattr(ds, "variable_names", None)
        trees = ts.parse_trees(tree_sorts) if tree_sorts else []
        if tree_chars:
            chars = [c.strip() for c in tree_chars.split(",") if c.strip()] if isinstance(tree_chars, str) else list(tree_chars)
            trees = trees + ts.all_trees(chars, tree_depth)
        if not trees:
            raise ValueError("tree sorts: no trees")
        if len(trees) > ts.MAX_TREES:
            raise ValueError(f"tree sorts: at most {ts.MAX_TREES} trees per call, got {len(trees)}")
        splits = ts.parse_tree_splits(tree_splits, len(trees[0]))
        if str(device).startswith("cuda"):
            wavg = average_weights(list(wdev[sort_split].cpu().numpy()), np_batches[sort_split]["mask"])
        else:
            wavg = average_weights([w[sort_split] for w in weights], np_batches[sort_split]["mask"])
        res_ts = ts.tree_sorted_portfolios(models, b, trees, splits=splits, device=device, names=names, weights=wavg)
        priced = ts.price_tree_sorted(res_ts, wavg, np_batches[sort_split]["returns"], np_batches[sort_split]["mask"])
        out["tree_sorts"] = {"portfolios": res_ts, "priced": priced}
        sx = " x ".join(str(q) for q in res_ts["splits"])
        say(bar); say(f"TREE-SORTED PORTFOLIOS ({sort_split} split, splits {sx}, equally weighted)")
        say(bar); say()
        for line in ts.format_tree_sorted(priced):
            say(line)
        say()
        if tree_out:
            with open(tree_out, "w") as fh:
                json.dump(ts.tree_to_json(res_ts, priced), fh, indent=1)
            say(f"  Saved: {tree_out}"); say()
        if tree_prune:
            from . import tree_prune as tp
            n0, n2, n1 = tp.parse_prune_grid(prune_grid)
            by_split = {sort_split: res_ts}
            ws_split = {sort_split: wavg}
            for s in SPLITS:
                if s in by_split:
                    continue
                if str(device).startswith("cuda"):
                    ws = average_weights(list(wdev[s].cpu().numpy()), np_batches[s]["mask"])
                else:
                    ws = average_weights([w[s] for w in weights], np_batches[s]["mask"])
                by_split[s] = ts.tree_sorted_portfolios(models, batches[s], trees, splits=splits, device=device, names=names,
                                                        weights=ws)
                ws_split[s] = ws
            pruned = tp.prune_trees(by_split, l0=tp.PRUNE_L0[:n0], l2_rel=tp.PRUNE_L2_REL[:n2], n1=n1,
                                    max_assets=prune_max_assets, device=device)
            out["tree_prune"] = pruned
            F = int(b["individual_features"].shape[2])
            kn = ([str(x) for x in names] if names is not None and len(names) == F else [str(j) for j in range(F)]) + ["weight"]
            say(bar); say(f"PRUNED TREES (elastic-net mean-variance SDF on the tree nodes, at most {int(prune_max_assets)})")
            say(bar); say()
            for line in tp.format_pruned(pruned, gan={k: res[k] for k in ("train_sharpe", "valid_sharpe", "test_sharpe")},
                                         key_names=kn):
                say(line)
            say()
            pmj = None
            if prune_metrics or prune_weights_out:
                pw = tp.pruned_weights(pruned, by_split, batches, models, device=device, weights=ws_split)
                pmx = tp.pruned_metrics(pruned, by_split, pw, batches)
                out["tree_prune_metrics"] = pmx
                pmj = {k: float(v) for k, v in pmx.items()}
                say(bar); say("PRUNED TREES: STOCK-LEVEL WEIGHTS (EV / XS-R2 / turnover / max 1-month loss, test split)")
                say(bar); say()
                for line in tp.format_pruned_metrics(pmx, gan=out["paper_metrics"]["test"] if paper else None):
                    say(line)
                say()
                if prune_weights_out:
                    np.savez(prune_weights_out, **{s: pw[s] for s in SPLITS})
                    say(f"  Saved: {prune_weights_out}"); say()
            if prune_out:
                pj = tp.pruned_to_json(pruned)
                if pmj is not None:
                    pj["tree_prune_metrics"] = pmj
                with open(prune_out, "w") as fh:
                    json.dump(pj, fh, indent=1)
                say(f"  Saved: {prune_out}"); say()
    pred_json = {}
    if benchmark_ffn and not benchmarks:
        raise ValueError("benchmark_ffn needs benchmarks (CLI: --benchmark_ffn with --benchmarks)")
    if benchmark_ipca and not benchmarks:
        raise ValueError("benchmark_ipca needs benchmarks (CLI: --benchmark_ipca with --benchmarks)")
    if benchmarks:
        from . import benchmarks as bm
        from .portfolio import cross_sectional_r2, explained_variation
        res_bm = bm.linear_benchmarks(batches, device=device, center=benchmark_center, grid=bm.parse_grid(benchmark_grid))
        tb = np_batches["test"]
        if str(device).startswith("cuda"):
            wavg = average_weights(list(wdev["test"].cpu().numpy()), tb["mask"])
        else:
            wavg = average_weights([w["test"] for w in weights], tb["mask"])
        gan = {"train_sharpe": res["train_sharpe"], "valid_sharpe": res["valid_sharpe"], "test_sharpe": res["test_sharpe"],
               "ev": explained_variation(wavg, tb["returns"], tb["mask"]),
               "xs_r2": cross_sectional_r2(wavg, tb["returns"], tb["mask"])}
        out["benchmarks"] = {"linear": res_bm, "gan": gan}
        ffn_kw = {}
        if benchmark_ffn:
            from . import prediction as pred
            ffn = pred.ffn_benchmark(batches, models[0].config, device=device, epochs=prediction_epochs,
                                     lr=prediction_lr, seeds=tuple(prediction_seeds))
            out["benchmarks"]["ffn"] = pred_json["FFN"] = ffn
            ffn_kw = {"ffn": ffn}
        if benchmark_ipca:
            from . import ipca as ip
            row = ip.ipca_benchmark(batches, factors=tuple(ipca_factors), intercept=ipca_intercept, device=device)
            out["benchmarks"]["ipca"] = row
            ffn_kw["ipca"] = row
        say(bar); say("BENCHMARK SDFS (linear LS / elastic net EN vs the ensemble)"); say(bar); say()
        for line in bm.format_benchmarks(res_bm, gan, **ffn_kw):
            say(line)
        say()
        if benchmarks_out:
            with open(benchmarks_out, "w") as fh:
                json.dump(bm.to_json(res_bm, gan, **ffn_kw), fh, indent=1)
            say(f"  Saved: {benchmarks_out}"); say()
    if fama_macbeth:
        from . import ipca as ip
        if sort_split not in SPLITS:
            raise ValueError(f"sort_split must be one of {SPLITS}")
        names = getattr(datasets[SPLITS.index(sort_split)], "variable_names", None)
        res_fm = ip.fama_macbeth(batches[sort_split], intercept=ipca_intercept, device=device)
        out["fama_macbeth"] = res_fm
        say(bar); say(f"FAMA-MACBETH REGRESSIONS ({sort_split} split)"); say(bar); say()
        for line in ip.format_fama_macbeth(res_fm, names):
            say(line)
        say()
        if fm_out:
            with open(fm_out, "w") as fh:
                json.dump(ip.fama_macbeth_json(res_fm, names), fh, indent=1)
            say(f"  Saved: {fm_out}"); say()
    if beta_network:
        from . import prediction as pred
        from .portfolio import cross_sectional_r2, explained_variation
        wavg, proxy = {}, {}
        for s in SPLITS:
            b = np_batches[s]
            if str(device).startswith("cuda"):
                wavg[s] = average_weights(list(wdev[s].cpu().numpy()), b["mask"])
            else:
                wavg[s] = average_weights([w[s] for w in weights], b["mask"])
            proxy[s] = {"ev": explained_variation(wavg[s], b["returns"], b["mask"]),
                        "xs_r2": cross_sectional_r2(wavg[s], b["returns"], b["mask"])}
        res_bn = pred.beta_network(wavg, batches, models[0].config, device=device, epochs=prediction_epochs,
                                   lr=prediction_lr, seeds=tuple(prediction_seeds))
        res_bn["proxy"] = proxy
        out["beta_network"] = pred_json["beta_network"] = res_bn
        say(bar); say("BETA NETWORK (EV / XS-R2 with fitted loadings vs the SDF-weight proxy)"); say(bar); say()
        for line in pred.format_beta(res_bn, proxy):
            say(line)
        say()
    if prediction_out and pred_json:
        from . import prediction as pred
        with open(prediction_out, "w") as fh:
            json.dump({k: pred.to_json(v) for k, v in pred_json.items()}, fh, indent=1)
        say(f"  Saved: {prediction_out}"); say()
    if weight_structure:
        from . import weight_structure as wst
        if structure_split not in SPLITS:
            raise ValueError(f"structure_split must be one of {SPLITS}")
        ds = datasets[SPLITS.index(structure_split)]
        b = batches[structure_split]
        names = getattr(ds, "variable_names", None)
        res_ws = wst.weight_structure(models, b, device=device, grid=wst.default_grid_base(b, int(structure_points))[0],
                                      pairs=wst.parse_pairs(structure_pairs, names), names=names)
        out["weight_structure"] = res_ws
        say(bar); say(f"WEIGHT STRUCTURE ({structure_split} split, ensemble weight)"); say(bar); say()
        for line in wst.format_structure(res_ws):
            say(line)
        say()
        if structure_out:
            with open(structure_out, "w") as fh:
                json.dump(wst.to_json(res_ws), fh, indent=1)
            say(f"  Saved: {structure_out}"); say()
    if knockout:
        from . import knockout as ko
        if knockout_split not in SPLITS:
            raise ValueError(f"knockout_split must be one of {SPLITS}")
        ds = datasets[SPLITS.index(knockout_split)]
        groups = ko.load_groups(knockout_groups) if isinstance(knockout_groups, str) else knockout_groups
        mkw = {}
        if knockout_macro or knockout_macro_groups:
            mg = ko.load_groups(knockout_macro_groups) if isinstance(knockout_macro_groups, str) else knockout_macro_groups
            mkw = dict(macro=bool(knockout_macro), macro_groups=mg, macro_base=knockout_macro_base,
                       macro_names=getattr(ds, "macro_names", None))
        rep = ko.knockout_importance(models, batches[knockout_split], groups=groups, base=knockout_base,
                                     xs_r2=knockout_xs_r2, device=device, names=getattr(ds, "variable_names", None),
                                     **mkw)
        out["knockout"] = rep
        what = "CHARACTERISTIC AND MACRO KNOCK-OUTS" if "macro_columns" in rep else "CHARACTERISTIC KNOCK-OUTS"
        say(bar); say(f"{what} ({knockout_split} split, ensemble SDF, {rep['path']} path)")
        say(bar); say()
        for line in ko.format_knockout(rep):
            say(line)
        say()
        if knockout_out:
            with open(knockout_out, "w") as fh:
                json.dump(ko.to_json(rep), fh, indent=1)
            say(f"  Saved: {knockout_out}"); say()
    return out


def _parser():
    p = argparse.ArgumentParser(description="Evaluate an ensemble by averaging SDF weights")
    p.add_argument("--data_dir", type=str, required=True)
    p.add_argument("--checkpoint_dirs", type=str, nargs="+", required=True)
    p.add_argument("--device", type=str, default="cpu", help="cpu | cuda (batched native engine)")
    p.add_argument("--paper_metrics", action="store_true", help="also print EV / XS-R2 / turnover / max loss")
    p.add_argument("--variable_importance", action="store_true",
                   help="also print the sensitivity ranking of the ensemble weight")
    p.add_argument("--importance_split", type=str, default="test", choices=SPLITS)
    p.add_argument("--importance_out", type=str, default=None, help="write the ranking to FILE.json")
    p.add_argument("--importance_macro_lags", type=int, default=0,
                   help="with --variable_importance: also rank the macro series through the LSTM, lags 0..L-1")
    p.add_argument("--sorted_portfolios", action="store_true",
                   help="also price the quantile portfolios sorted on every characteristic and on the weight")
    p.add_argument("--sort_split", type=str, default="test", choices=SPLITS)
    p.add_argument("--sort_quantiles", type=int, default=10, help="buckets per sort (2..16)")
    p.add_argument("--sort_out", type=str, default=None, help="write the sorted-portfolio results to FILE.json")
    p.add_argument("--weight_structure", action="store_true",
                   help="also compute the response curves (and surfaces) of the ensemble weight")
    p.add_argument("--structure_split", type=str, default="test", choices=SPLITS)
    p.add_argument("--structure_points", type=int, default=21, help="grid points per characteristic (2..64)")
    p.add_argument("--structure_pairs", type=str, default=None,
                   help="interaction surfaces: 'all' or a comma list of A:B, by name or column index")
    p.add_argument("--structure_out", type=str, default=None, help="write the curves and surfaces to FILE.json")
    p.add_argument("--double_sorts", type=str, default=None,
                   help="double-sorted portfolios on --sort_split: a comma list of A:B, by name, column index or 'weight'")
    p.add_argument("--double_quantiles", type=str, default="5x5", help="QAxQB buckets (2..16 each, at most 36 cells)")
    p.add_argument("--double_mode", type=str, default="conditional", choices=("conditional", "independent"))
    p.add_argument("--double_out", type=str, default=None, help="write the double-sorted results to FILE.json")
    p.add_argument("--tree_sorts", type=str, default=None,
                   help="tree-sorted portfolios on --sort_split: a comma list of A:B:C, by name, column index or 'weight'")
    p.add_argument("--tree_chars", type=str, default=None,
                   help="every ordered sequence of --tree_depth of these keys (a comma list), the asset-pricing-tree set")
    p.add_argument("--tree_depth", type=int, default=3, help="depth of the --tree_chars trees (1..5)")
    p.add_argument("--tree_splits", type=str, default="2",
                   help="children per node: one integer for every level, or Q1xQ2x.. (2..16 each, at most 36 leaves)")
    p.add_argument("--tree_out", type=str, default=None, help="write the tree-sorted results to FILE.json")
    p.add_argument("--tree_prune", action="store_true",
                   help="with --tree_sorts / --tree_chars: prune the tree nodes into a sparse mean-variance SDF (elastic net)")
    p.add_argument("--prune_max_assets", type=int, default=40, help="nodes of the pruned SDF at most")
    p.add_argument("--prune_grid", type=str, default="3x3x16", help="penalties N0xN2xN1 of l0 (<= 3) x l2 (<= 3) x l1")
    p.add_argument("--prune_out", type=str, default=None, help="write the pruning results to FILE.json")
    p.add_argument("--prune_metrics", action="store_true",
                   help="with --tree_prune: stock-level weights of the pruned SDF, its EV / XS-R2 / turnover / max loss")
    p.add_argument("--prune_weights_out", type=str, default=None,
                   help="with --prune_metrics: save the dense weights of the three splits to FILE.npz")
    p.add_argument("--benchmarks", action="store_true",
                   help="also evaluate the linear (LS) and elastic-net (EN) benchmark SDFs next to the ensemble")
    p.add_argument("--benchmark_grid", type=str, default="16x4", help="EN penalties: N1xN2 values of l1 x l2 (N2 <= 4)")
    p.add_argument("--benchmark_center", type=str, default="mean", choices=("mean", "none"))
    p.add_argument("--benchmarks_out", type=str, default=None, help="write the benchmark results to FILE.json")
    p.add_argument("--benchmark_ffn", action="store_true",
                   help="with --benchmarks: also fit the FFN return-prediction benchmark (a row between EN and the ensemble)")
    p.add_argument("--beta_network", action="store_true",
                   help="also fit the beta network to the ensemble's SDF factor and print EV / XS-R2 with its loadings")
    p.add_argument("--prediction_epochs", type=int, default=64, help="fit epochs of the FFN benchmark / beta network")
    p.add_argument("--prediction_lr", type=float, default=None, help="their learning rate (default: 1e-3)")
    p.add_argument("--prediction_seeds", type=int, nargs="+", default=[0], help="their seeds (predictions are averaged)")
    p.add_argument("--prediction_out", type=str, default=None, help="write the FFN / beta-network results to FILE.json")
    p.add_argument("--benchmark_ipca", action="store_true",
                   help="with --benchmarks: also estimate the IPCA benchmark (a row between EN and FFN)")
    p.add_argument("--ipca_factors", type=int, nargs="+", default=[1, 2, 3, 4, 5, 6],
                   help="candidate numbers of IPCA factors (selected on the validation split)")
    p.add_argument("--ipca_no_intercept", action="store_true",
                   help="IPCA / Fama-MacBeth without the constant column")
    p.add_argument("--fama_macbeth", action="store_true",
                   help="also print the Fama-MacBeth slope table of --sort_split")
    p.add_argument("--fm_out", type=str, default=None, help="write the Fama-MacBeth table to FILE.json")
    p.add_argument("--knockout", action="store_true",
                   help="also print what the ensemble SDF loses without each characteristic (and each group)")
    p.add_argument("--knockout_split", type=str, default="test", choices=SPLITS)
    p.add_argument("--knockout_groups", type=str, default=None,
                   help="FILE.json: {group name: [columns or characteristic names]}, one scenario per group")
    p.add_argument("--knockout_base", type=str, default="zero", choices=("zero", "median"))
    p.add_argument("--knockout_xs_r2", action="store_true", help="with --knockout: also XS-R2 per scenario")
    p.add_argument("--knockout_out", type=str, default=None, help="write the knock-out report to FILE.json")
    p.add_argument("--knockout_macro", action="store_true",
                   help="with --knockout: also one scenario per macro series, held constant over the split, through the LSTM")
    p.add_argument("--knockout_macro_groups", type=str, default=None,
                   help="with --knockout: FILE.json: {group name: [macro series or names]}, one scenario per group")
    p.add_argument("--knockout_macro_base", type=str, default="zero", choices=("zero", "median"),
                   help="with --knockout: the value a knocked-out series is held at (zero: the training mean)")
    return p


def _extra_kwargs(a) -> Dict:
    """The optional blocks' keyword arguments of ``evaluate_ensemble`` from the parsed flags."""
    kw = {"importance_macro_lags": a.importance_macro_lags} if a.importance_macro_lags else {}
    if a.weight_structure:
        kw.update(weight_structure=True, structure_split=a.structure_split, structure_points=a.structure_points,
                  structure_pairs=a.structure_pairs, structure_out=a.structure_out)
    if a.sorted_portfolios:
        kw.update(sorted_portfolios=True, sort_split=a.sort_split, sort_quantiles=a.sort_quantiles, sort_out=a.sort_out)
    if a.double_sorts:
        from .sorted_portfolios import parse_double_quantiles
        kw.update(double_sorts=a.double_sorts, double_quantiles=parse_double_quantiles(a.double_quantiles),
                  double_mode=a.double_mode, double_out=a.double_out, sort_split=a.sort_split)
    if a.tree_sorts or a.tree_chars:
        kw.update(tree_sorts=a.tree_sorts, tree_chars=a.tree_chars, tree_depth=a.tree_depth, tree_splits=a.tree_splits,
                  tree_out=a.tree_out, sort_split=a.sort_split)
    if a.tree_prune:
        if not (a.tree_sorts or a.tree_chars):
            raise SystemExit("--tree_prune needs --tree_sorts or --tree_chars")
        kw.update(tree_prune=True, prune_max_assets=a.prune_max_assets, prune_grid=a.prune_grid, prune_out=a.prune_out)
    if a.prune_metrics or a.prune_weights_out:
        if not a.tree_prune:
            raise SystemExit("--prune_metrics needs --tree_prune")
        if not a.prune_metrics:
            raise SystemExit("--prune_weights_out needs --prune_metrics")
        kw.update(prune_metrics=True, prune_weights_out=a.prune_weights_out)
    if a.benchmarks:
        from .benchmarks import parse_grid
        kw.update(benchmarks=True, benchmark_grid=parse_grid(a.benchmark_grid), benchmark_center=a.benchmark_center,
                  benchmarks_out=a.benchmarks_out)
    if a.benchmark_ffn or a.beta_network:
        if a.benchmark_ffn and not a.benchmarks:
            raise SystemExit("--benchmark_ffn needs --benchmarks")
        kw.update(benchmark_ffn=a.benchmark_ffn, beta_network=a.beta_network, prediction_epochs=a.prediction_epochs,
                  prediction_lr=a.prediction_lr, prediction_seeds=tuple(a.prediction_seeds),
                  prediction_out=a.prediction_out)
    if a.benchmark_ipca:
        if not a.benchmarks:
            raise SystemExit("--benchmark_ipca needs --benchmarks")
        kw.update(benchmark_ipca=True, ipca_factors=tuple(a.ipca_factors), ipca_intercept=not a.ipca_no_intercept)
    if a.fama_macbeth:
        kw.update(fama_macbeth=True, fm_out=a.fm_out, sort_split=a.sort_split, ipca_intercept=not a.ipca_no_intercept)
    if (a.knockout_macro or a.knockout_macro_groups or a.knockout_macro_base != "zero") and not a.knockout:
        raise SystemExit("--knockout_macro, --knockout_macro_groups and --knockout_macro_base need --knockout")
    if a.knockout:
        kw.update(knockout=True, knockout_split=a.knockout_split, knockout_groups=a.knockout_groups,
                  knockout_base=a.knockout_base, knockout_xs_r2=a.knockout_xs_r2, knockout_out=a.knockout_out)
        if a.knockout_macro or a.knockout_macro_groups:
            kw.update(knockout_macro=a.knockout_macro, knockout_macro_groups=a.knockout_macro_groups,
                      knockout_macro_base=a.knockout_macro_base)
    return kw


def main(argv=None):
    a = _parser().parse_args(argv)
    kw = _extra_kwargs(a)
    return evaluate_ensemble(a.checkpoint_dirs, a.data_dir, a.device, paper=a.paper_metrics,
                             importance=a.variable_importance, importance_split=a.importance_split,
                             importance_out=a.importance_out, **kw)


if __name__ == "__main__":
    main()
