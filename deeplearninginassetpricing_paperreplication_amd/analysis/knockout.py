"""Characteristic knock-outs: what the ensemble SDF loses, in Sharpe ratio and explained variation,
when a characteristic or a group of them is taken away from the trained models.

A scenario ``k`` is a set ``S_k`` of characteristic columns in ``0..F-1`` and a shared base row
``base[0..F-1]``; the empty set is the baseline. The counterfactual panel is ``x^k[t,i,c] = base[c]``
for ``c in S_k`` and ``x[t,i,c]`` otherwise; the state columns (LSTM output or raw macro) are
untouched. For member ``g`` of ``G`` in evaluation mode, per period ``t`` over its ``n_t`` valid rows:

    w_g      raw tower output on x^k                                            (fp32)
    c_g[t]   = fp32(sum_i w_g / max(n_t,1)) if normalize_w else 0               (zero_mean_normalize)
    v_g      = fp32(w_g - c_g[t])
    SA_g[t]  = sum_i |v_g|     SR_g[t] = sum_i v_g R     S1_g[t] = sum_i w_g    (fp64)
    e_i      = sum_g v_g,i * fp32(1 / (G * max(fp32(SA_g[t]), 1e-8)))           (fp32, fma in g order)
    EA[t] = sum_i |e|    E2[t] = sum_i e^2    ER[t] = sum_i e R                 (fp64)
    once per split:  n[t], sum_r[t], sum_rr[t]

(the quotients of ``c`` and of the scale are formed in fp64 and rounded once). Everything else is
host arithmetic on these sums:

  * ensemble factor ``F_t = -ER / EA``, or ``-ER`` where ``EA <= 1e-8`` (the rule of
    ``portfolio.renormalize`` with the paper sign of ``ensemble_sharpes``); every period of the split
    counts, an empty one gives 0;
  * member factor ``-SR_g / max(SA_g, 1e-8)``; Sharpe ratios by ``sharpe_ddof0``;
  * ``EV = 1 - sum_t[(sum_rr - ER^2 / E2) / max(n,1)] / sum_t[sum_rr / max(n,1)]``, the
    ``explained_variation`` of the ensemble weights as loadings;
  * XS-R² needs per-stock sums: it comes from the dense ensemble weights ``e / EA`` of a scenario
    (``xs_r2=True``), fed to ``cross_sectional_r2``.

``knockout_importance`` reports, per scenario, Sharpe, EV, optionally XS-R², the member Sharpes and
the differences from the baseline (``d_sharpe``, ``d_ev``, ``d_xs_r2``), ranked by Sharpe loss.
Default scenarios: the baseline plus one per characteristic; ``groups`` (name -> columns or names)
adds one per group. ``base``: ``"zero"`` (the cross-sectional median of rank-normalised
characteristics), ``"median"`` (per-column median of the split's valid values, as
``weight_structure`` computes it) or an ``[F]`` array.

``device="cpu"`` loops over the scenarios with the PyTorch tower (any architecture, mixed ensembles,
``dtype``; float32 applies the roundings above, float64 none of them). ``device="cuda"`` runs
``csrc/k_knock.hip`` through ``Engine.knockout``: every panel tile is read once per member and
evaluated under all scenarios, and the ensemble factor is reduced per scenario without a dense
intermediate. Mixed-architecture ensembles and shapes the kernel does not cover (the wide layer-0
path) fall back to the CPU path with a printed note; a split the engine cannot hold (more periods
than it accepts, and ``Engine.knockout`` itself takes at most 65535) raises ``ValueError``.

Macro knock-outs (``macro=True``, ``macro_groups``, ``extra_scenarios``). A scenario also holds a set
``Q_k`` of macro series in ``0..M-1`` and the shared base row ``macro_base[0..M-1]``. The counterfactual
split has ``x^k`` as above and

    m^k[t][j] = macro_base[j]  for j in Q_k, every period t of the split;   m[t][j] otherwise
    pp_g^k    = member g's evaluation LSTM run over m^k[0..T-1] from the state the split's evaluation
                starts from, every layer, evaluation mode; without an LSTM pp_g^k[t] = m^k[t]
    w_g       = raw tower output on (x^k, pp_g^k)           -- everything after this line is as above

``macro`` is the standardised series the model is fed, so ``macro_base="zero"`` (the default) is the
training mean; ``"median"`` is the per-series median over the split's periods; or an ``[M]`` array. A
knock-out holds a series constant over the whole split: the question is what the trained ensemble does
in a world where the series carries no information. The moment network, the train statistics and the
split's length are untouched. The scenario order is: baseline, characteristic singles, characteristic
groups, macro singles, macro groups, ``extra_scenarios`` -- ``(label, columns, macro_columns)``, the
only way to a scenario that replaces characteristics and series together. When a macro scenario is
present the report gains ``macro_columns`` (one list per scenario) and ``macro_base``; without one it is
key for key and bit for bit the characteristic report. ``device="cuda"`` then runs
``Engine.knockout_macro``: per (scenario, member) the forward's own projection and recurrence kernels
over the altered series, and ``k_knock_fwd_pp``, which inserts the scenario's per-period table into
tiles it loaded once. A model set without macro input raises ``ValueError``.

Out of scope: knock-outs over a window of periods or at a lag, knocking out the LSTM state columns of
an LSTM model, sharing a recurrence between scenarios, the moment network and its LSTM, retraining
without a characteristic or a series, multi-rank runs, a shipped category map (the groups file is the
user's).
"""
from __future__ import annotations

import copy
import json
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .importance import _state
from .portfolio import cross_sectional_r2, sharpe_ddof0
from .weight_structure import _tower

SUM_KEYS = ("EA", "E2", "ER", "S1", "SA", "SR")


# ---- scenarios ----------------------------------------------------------------------------------
def _column(tok, F: int, idx: Dict[str, int]) -> int:
    if isinstance(tok, str):
        if tok in idx:
            return idx[tok]
        try:
            c = int(tok)
        except ValueError:
            raise ValueError(f"knockout: unknown characteristic {tok!r}") from None
    else:
        c = int(tok)
    if c < 0 or c >= F:
        raise ValueError(f"knockout: column {c} outside [0, {F})")
    return c


def build_scenarios(F: int, groups=None, names: Optional[Sequence] = None, singles: bool = True):
    """(labels, columns): the baseline, one scenario per characteristic (``singles``), one per group."""
    nm = [str(n) for n in names] if names is not None and len(names) == F else [f"x{j}" for j in range(F)]
    idx = {n: j for j, n in enumerate(nm)}
    labels, cols = ["baseline"], [()]
    if singles:
        labels += nm
        cols += [(j,) for j in range(F)]
    if groups:
        if not isinstance(groups, dict):
            raise ValueError("knockout: groups must map a name to a list of columns or names")
        for g, members in groups.items():
            if isinstance(members, (str, int)) or len(members) == 0:
                raise ValueError(f"knockout: group {g!r} must be a non-empty list of columns or names")
            cs = tuple(sorted({_column(m, F, idx) for m in members}))
            labels.append(str(g))
            cols.append(cs)
    return labels, cols


def _macro_column(tok, M: int, idx: Dict[str, int]) -> int:
    if isinstance(tok, str):
        if tok in idx:
            return idx[tok]
        try:
            c = int(tok)
        except ValueError:
            raise ValueError(f"knockout: unknown macro series {tok!r}") from None
    else:
        c = int(tok)
    if c < 0 or c >= M:
        raise ValueError(f"knockout: macro series {c} outside [0, {M})")
    return c


def macro_series_names(M: int, macro_names: Optional[Sequence] = None) -> List[str]:
    """The names the macro importance report uses: ``macro_names`` when it has M entries, else macro0.."""
    return [str(n) for n in macro_names] if macro_names is not None and len(macro_names) == M \
        else [f"macro{j}" for j in range(M)]


def build_macro_scenarios(M: int, macro_groups=None, macro_names: Optional[Sequence] = None, singles: bool = True):
    """(labels, macro_columns): one scenario per macro series (``singles``), one per group; no baseline."""
    nm = macro_series_names(M, macro_names)
    idx = {n: j for j, n in enumerate(nm)}
    labels, cols = [], []
    if singles:
        labels += nm
        cols += [(j,) for j in range(M)]
    if macro_groups:
        if not isinstance(macro_groups, dict):
            raise ValueError("knockout: macro_groups must map a name to a list of series or names")
        for g, members in macro_groups.items():
            if isinstance(members, (str, int)) or len(members) == 0:
                raise ValueError(f"knockout: macro group {g!r} must be a non-empty list of series or names")
            labels.append(str(g))
            cols.append(tuple(sorted({_macro_column(m, M, idx) for m in members})))
    return labels, cols


def _macro_dim(batch: Dict) -> int:
    mac = batch.get("macro_features")
    return 0 if mac is None else int(mac.shape[-1])


def resolve_macro_base(macro_base, batch: Dict) -> np.ndarray:
    M = _macro_dim(batch)
    if isinstance(macro_base, str):
        if macro_base == "zero":
            return np.zeros(M)
        if macro_base == "median":
            mac = batch["macro_features"]
            mac = mac.cpu().numpy() if isinstance(mac, torch.Tensor) else np.asarray(mac)
            return np.median(mac.astype(np.float64), axis=0) if mac.shape[0] else np.zeros(M)
        raise ValueError("knockout: macro_base must be 'zero', 'median' or an [M] array")
    b = np.asarray(macro_base, dtype=np.float64).ravel()
    if len(b) != M:
        raise ValueError(f"knockout: macro_base must have M = {M} entries")
    return b


def resolve_base(base, batch: Dict) -> np.ndarray:
    F = int(batch["individual_features"].shape[-1])
    if isinstance(base, str):
        if base == "zero":
            return np.zeros(F)
        if base == "median":
            from .weight_structure import default_grid_base
            return np.asarray(default_grid_base(batch)[1], dtype=np.float64)
        raise ValueError("knockout: base must be 'zero', 'median' or an [F] array")
    b = np.asarray(base, dtype=np.float64).ravel()
    if len(b) != F:
        raise ValueError(f"knockout: base must have F = {F} entries")
    return b


def scenario_masks(cols: Sequence[Sequence[int]], F: int) -> np.ndarray:
    """uint32 [K][ceil(F / 32)]: bit c % 32 of word c / 32 is set for the columns of the scenario."""
    m = np.zeros((len(cols), (F + 31) // 32), dtype=np.uint32)
    for k, cs in enumerate(cols):
        for c in cs:
            if c < 0 or c >= F:
                raise ValueError(f"knockout: column {c} outside [0, {F})")
            m[k, c // 32] |= np.uint32(1 << (c % 32))
    return m


def macro_scenario_masks(macro_cols: Sequence[Sequence[int]], M: int) -> np.ndarray:
    """uint32 [K][ceil(M / 32)]: bit j % 32 of word j / 32 is set for the macro series of the scenario."""
    m = np.zeros((len(macro_cols), (M + 31) // 32), dtype=np.uint32)
    for k, q in enumerate(macro_cols):
        for j in q:
            if j < 0 or j >= M:
                raise ValueError(f"knockout: macro series {j} outside [0, {M})")
            m[k, j // 32] |= np.uint32(1 << (j % 32))
    return m


# ---- the definition, from raw weights -----------------------------------------------------------
def knockout_sums_numpy(w, returns, mask, normalize_w=True, dtype=np.float64, dense: bool = False) -> Dict:
    """The sums of the module docstring from raw weights ``w`` [K][G][T][N] (values at masked
    entries are ignored). ``normalize_w``: a flag, or one per member. ``dtype=np.float32`` applies
    the stated fp32 roundings (the fma is formed in float64 and rounded once more, which differs
    from a fused one only where the float64 sum falls on a float32 tie); ``np.float64`` applies none.
    ``dense=True`` adds ``dense`` [K][T][N] = e / EA (e where EA <= 1e-8), zero at masked entries."""
    w = np.asarray(w)
    K, G, T, N = w.shape
    f32 = np.dtype(dtype) == np.float32
    ft = np.float32 if f32 else np.float64
    m = np.asarray(mask).astype(bool)
    md = m.astype(np.float64)
    R = np.where(m, np.asarray(returns, dtype=np.float64), 0.0)
    n = md.sum(1)
    norm = np.broadcast_to(np.asarray(normalize_w, dtype=bool), (G,))
    wv = np.where(m, w.astype(ft), ft(0))                                   # [K][G][T][N]
    S1 = wv.astype(np.float64).sum(3)                                       # [K][G][T]
    c = (S1 / np.maximum(n, 1.0)).astype(ft) * norm[None, :, None].astype(ft)
    v = np.where(m, (wv - c[..., None]).astype(ft), ft(0))
    vd = v.astype(np.float64)
    SA = np.abs(vd).sum(3)
    SR = (vd * R).sum(3)
    if f32:
        s = (1.0 / (G * np.maximum(SA.astype(np.float32), np.float32(1e-8)).astype(np.float64))).astype(np.float32)
    else:
        s = 1.0 / (G * np.maximum(SA, 1e-8))
    e = np.zeros((K, T, N), dtype=ft)
    for g in range(G):
        e = (vd[:, g] * s[:, g, :, None].astype(np.float64) + e.astype(np.float64)).astype(ft)
    ed = np.where(m, e.astype(np.float64), 0.0)
    out = {"n": n, "sum_r": R.sum(1), "sum_rr": (R * R).sum(1),
           "EA": np.abs(ed).sum(2), "E2": (ed * ed).sum(2), "ER": (ed * R).sum(2), "S1": S1, "SA": SA, "SR": SR}
    if dense:
        ea = out["EA"][..., None]
        out["dense"] = np.where(ea > 1e-8, ed / np.where(ea > 1e-8, ea, 1.0), ed)
    return out


def factor_series(sums: Dict) -> np.ndarray:
    """F [K][T] = -ER / EA, or -ER where EA <= 1e-8."""
    EA, ER = np.asarray(sums["EA"], dtype=np.float64), np.asarray(sums["ER"], dtype=np.float64)
    ok = EA > 1e-8
    return -np.where(ok, ER / np.where(ok, EA, 1.0), ER)


def metrics_from_knockout_sums(sums: Dict, dense=None, returns=None, mask=None) -> Dict:
    """sharpe [K], ev [K], member_sharpes [K][G], factor [K][T] from the sums; xs_r2 [K] where the
    dense ensemble weights [K][T][N] (with ``returns`` and ``mask``) are given, else None."""
    EA, E2, ER = (np.asarray(sums[k], dtype=np.float64) for k in ("EA", "E2", "ER"))
    SA, SR = np.asarray(sums["SA"], dtype=np.float64), np.asarray(sums["SR"], dtype=np.float64)
    n = np.maximum(np.asarray(sums["n"], dtype=np.float64), 1.0)
    srr = np.asarray(sums["sum_rr"], dtype=np.float64)
    K, G = SA.shape[:2]
    F = factor_series(sums)
    mf = -SR / np.maximum(SA, 1e-8)
    # explained_variation of the weights e / EA (e where EA <= 1e-8): beta = rw / ww where ww > 1e-12
    den_w = np.where(EA > 1e-8, EA, 1.0)
    ok = E2 / (den_w * den_w) > 1e-12
    resid = srr[None] - np.where(ok, ER * ER / np.where(ok, E2, 1.0), 0.0)
    den = float((srr / n).sum())
    ev = 1.0 - (resid / n[None]).sum(1) / den if den > 0 else np.full(K, np.nan)
    xs = None
    if dense is not None:
        r, m = np.asarray(returns), np.asarray(mask)
        xs = np.array([cross_sectional_r2(np.asarray(dense[k], dtype=np.float64), r, m) for k in range(K)])
    return {"sharpe": np.array([sharpe_ddof0(F[k]) for k in range(K)]), "ev": np.asarray(ev, dtype=np.float64),
            "xs_r2": xs, "member_sharpes": np.array([[sharpe_ddof0(mf[k, g]) for g in range(G)] for k in range(K)]),
            "factor": F}


# ---- the two paths ------------------------------------------------------------------------------
def raw_weights_cpu(ms, batch, cols: Sequence[int], base: np.ndarray, dtype, macro_cols: Sequence[int] = (),
                    macro_base: Optional[np.ndarray] = None) -> np.ndarray:
    """[G][T][N] raw tower outputs of the (prepared) models on the batch with ``cols`` set to base and
    the macro series ``macro_cols`` set to ``macro_base`` in every period."""
    feats = batch["individual_features"].to(dtype)
    macro = batch.get("macro_features")
    macro = None if macro is None else macro.to(dtype)
    if len(macro_cols):
        if macro is None:
            raise ValueError("knockout: a macro scenario needs macro_features")
        macro = macro.clone()
        macro[:, list(macro_cols)] = torch.as_tensor(np.asarray(macro_base)[list(macro_cols)]).to(dtype)
    T, N, F = feats.shape
    x = feats
    if len(cols):
        x = feats.clone()
        x[:, :, list(cols)] = torch.as_tensor(base[list(cols)]).to(dtype)
    out = []
    for m in ms:
        st = _state(m, macro)
        with torch.no_grad():
            xi = x if st is None else torch.cat([x, st[:, None, :].expand(T, N, st.shape[-1])], -1)
            out.append(_tower(m, xi.reshape(T * N, -1)).reshape(T, N).numpy())
    return np.stack(out)


def _cpu_sums(models, batch, cols, base, dtype, dense: bool, macro_cols=None, macro_base=None) -> Dict:
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    ms = [copy.deepcopy(m).cpu().to(dtype).eval() for m in models]
    norm = [bool(m.sdf_net.normalize_weights) for m in ms]
    nd = np.float32 if dtype == torch.float32 else np.float64
    ret, mask = cpu["returns"].numpy(), cpu["mask"].bool().numpy()
    parts = []
    for k, cs in enumerate(cols):                   # one scenario at a time: [1][G][T][N] in memory
        w = raw_weights_cpu(ms, cpu, cs, base, dtype, macro_cols[k] if macro_cols else (), macro_base)
        parts.append(knockout_sums_numpy(w[None], ret, mask, norm, nd, dense))
    out = {k: parts[0][k] for k in ("n", "sum_r", "sum_rr")}
    for k in SUM_KEYS + (("dense",) if dense else ()):
        out[k] = np.concatenate([p[k] for p in parts], 0)
    return out


def _gpu_sums(models, batch, cols, base, precision: str, dense: bool, macro_cols=None, macro_base=None) -> Optional[Dict]:
    """The same sums from the native engine, or None (with a printed note) where it does not apply.
    ``Engine.knockout_macro`` is used only when a macro scenario is present."""
    has_macro = bool(macro_cols) and any(len(q) for q in macro_cols)
    if len({m.spec for m in models}) != 1:
        print("[knockout] mixed-architecture ensemble: using the CPU path")
        return None
    from ..engine.runner import GANEngine
    F = int(batch["individual_features"].shape[-1])
    T, N = batch["mask"].shape
    K = len(cols)
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = GANEngine(models[0].spec, len(models), max_epochs=4, precision=precision)
    eng.set_data(batch)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    e = eng.eng
    try:
        if not e.knockout_supported(0):
            print("[knockout] knockout: not available for this shape: using the CPU path")
            return None
        if has_macro and not e.knockout_macro_supported(0):
            print("[knockout] knockout_macro: not available for this shape: using the CPU path")
            return None
        wd = torch.zeros(K, T, N, dtype=torch.float32, device=dev) if dense else None
        torch.cuda.synchronize(dev)
        try:
            if has_macro:
                M = _macro_dim(batch)
                r = e.knockout_macro(0, scenario_masks(cols, F), macro_scenario_masks(macro_cols, M), K,
                                     [float(x) for x in np.asarray(base, dtype=np.float32)],
                                     [float(x) for x in np.asarray(macro_base, dtype=np.float32)],
                                     wd.data_ptr() if dense else 0)
            else:
                r = e.knockout(0, scenario_masks(cols, F), K, [float(x) for x in np.asarray(base, dtype=np.float32)],
                               wd.data_ptr() if dense else 0)
        except ValueError as err:
            print(f"[knockout] {err}: using the CPU path")
            return None
    finally:
        e.sync()
    out = {k: np.asarray(r[k], dtype=np.float64) for k in ("n", "sum_r", "sum_rr") + SUM_KEYS}
    out["gpu_ms"] = (float(r["fwd_ms"]), float(r["reduce_ms"]))
    if has_macro:
        out["gpu_ms"] += (float(r["lstm_ms"]),)
    if dense:
        out["dense"] = wd.cpu().numpy()
    return out


def knockout_importance(models: Sequence, batch: Dict, groups=None, base="zero", xs_r2: bool = False,
                        device: str = "cpu", precision: str = "bf16", dtype: torch.dtype = torch.float32,
                        names: Optional[Sequence] = None, singles: bool = True, macro: bool = False,
                        macro_groups=None, macro_base="zero", macro_names: Optional[Sequence] = None,
                        macro_singles: bool = True, extra_scenarios=None) -> Dict:
    """The knock-out report of the ensemble over ``batch`` (module docstring): ``scenarios`` (labels),
    ``columns``, ``sharpe`` / ``ev`` / ``xs_r2`` [K] (``xs_r2`` None unless asked for), ``member_sharpes``
    [K][G], ``d_sharpe`` / ``d_ev`` / ``d_xs_r2`` (scenario minus baseline), ``factor`` [K][T],
    ``ranking`` (the scenarios other than the baseline, largest Sharpe loss first), ``base`` and
    ``path`` (``"engine"`` or ``"cpu"``). ``precision`` applies to the engine, ``dtype`` to the CPU path.
    ``macro=True`` adds one scenario per macro series (``macro_singles``) and one per entry of
    ``macro_groups``; ``extra_scenarios`` a list of ``(label, columns, macro_columns)``. With a macro
    scenario present the report also has ``macro_columns`` and ``macro_base`` (module docstring)."""
    models = list(models)
    if not models:
        raise ValueError("no models")
    F = int(batch["individual_features"].shape[-1])
    labels, cols = build_scenarios(F, groups, names, singles)
    b = resolve_base(base, batch)
    qcols, mb = None, None
    if macro or macro_groups or extra_scenarios:
        M = _macro_dim(batch)
        qcols = [()] * len(cols)
        no_macro = M == 0 or any(int(m.sdf_net.macro_dim) == 0 for m in models)
        if (macro or macro_groups) and no_macro:
            raise ValueError("knockout: a macro scenario needs models with macro input (macro_feature_dim > 0)")
        if macro or macro_groups:
            ql, qc = build_macro_scenarios(M, macro_groups, macro_names, macro_singles and bool(macro))
            labels, cols, qcols = labels + ql, cols + [()] * len(qc), qcols + qc
        if extra_scenarios:
            cn = [str(n) for n in names] if names is not None and len(names) == F else [f"x{j}" for j in range(F)]
            cidx = {n: j for j, n in enumerate(cn)}
            midx = {n: j for j, n in enumerate(macro_series_names(M, macro_names))}
            for item in extra_scenarios:
                if len(item) != 3:
                    raise ValueError("knockout: an extra scenario is (label, columns, macro_columns)")
                lab, cs, qs = item
                labels.append(str(lab))
                cols.append(tuple(sorted({_column(c, F, cidx) for c in cs})))
                qcols.append(tuple(sorted({_macro_column(q, M, midx) for q in qs})))
        if any(len(q) for q in qcols):
            if no_macro:
                raise ValueError("knockout: a macro scenario needs models with macro input (macro_feature_dim > 0)")
            mb = resolve_macro_base(macro_base, batch)
        else:
            qcols = None
    sums = None
    if str(device).startswith("cuda"):
        sums = _gpu_sums(models, batch, cols, b, precision, xs_r2, qcols, mb)
    path = "engine" if sums is not None else "cpu"
    if sums is None:
        sums = _cpu_sums(models, batch, cols, b, dtype, xs_r2, qcols, mb)
    ret = batch["returns"].cpu().numpy() if isinstance(batch["returns"], torch.Tensor) else np.asarray(batch["returns"])
    msk = batch["mask"].cpu().numpy() if isinstance(batch["mask"], torch.Tensor) else np.asarray(batch["mask"])
    met = metrics_from_knockout_sums(sums, sums.get("dense"), ret, msk)
    out = {"scenarios": labels, "columns": [list(c) for c in cols], "sharpe": met["sharpe"], "ev": met["ev"],
           "xs_r2": met["xs_r2"], "member_sharpes": met["member_sharpes"], "factor": met["factor"],
           "d_sharpe": met["sharpe"] - met["sharpe"][0], "d_ev": met["ev"] - met["ev"][0],
           "d_xs_r2": None if met["xs_r2"] is None else met["xs_r2"] - met["xs_r2"][0],
           "base": b, "path": path, "sums": {k: sums[k] for k in ("n", "sum_r", "sum_rr") + SUM_KEYS}}
    if qcols is not None:
        out["macro_columns"] = [list(q) for q in qcols]
        out["macro_base"] = mb
    rest = np.arange(1, len(labels))
    out["ranking"] = [int(k) for k in rest[np.argsort(out["d_sharpe"][1:], kind="stable")]]
    return out


def format_knockout(rep: Dict, top: int = 20) -> List[str]:
    """The printed table: scenario, Sharpe, d Sharpe, EV, d EV -- the baseline, then by Sharpe loss."""
    lines = [f"  {'scenario':<20s} {'Sharpe':>9s} {'d Sharpe':>9s} {'EV':>9s} {'d EV':>9s}"]
    for k in [0] + list(rep["ranking"][:top]):
        lines.append(f"  {rep['scenarios'][k]:<20s} {rep['sharpe'][k]:9.4f} {rep['d_sharpe'][k]:+9.4f} "
                     f"{rep['ev'][k]:9.4f} {rep['d_ev'][k]:+9.4f}")
    return lines


def to_json(rep: Dict) -> Dict:
    out = {}
    for k, v in rep.items():
        if k == "sums":
            continue
        out[k] = v.tolist() if isinstance(v, np.ndarray) else v
    return out


def load_groups(path: str) -> Dict:
    with open(path) as fh:
        g = json.load(fh)
    if not isinstance(g, dict):
        raise ValueError("knockout: the groups file must hold a JSON object: name -> list of columns or names")
    return g
