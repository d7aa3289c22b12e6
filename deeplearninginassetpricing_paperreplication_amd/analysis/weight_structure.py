"""Structure of the SDF weight (the paper's "SDF structure" figures): the weight as a function of
one characteristic (response curves) and of two characteristics at once (interaction surfaces),
every other characteristic held at a base value.

Inputs: ``G`` models of one ensemble, a split of ``T`` periods, for model ``g`` and period ``t``
the per-period tower inputs ``pp_g[t]`` (the evaluation LSTM's output, or the raw macro columns
without an LSTM: ``analysis.importance._state``), a grid ``u[0..P-1]`` (``P`` in 2..64), a base row
``x0[0..F-1]``, a scale table ``s[g][t]`` and items ``(a, b)``: ``b = -1`` is a curve over column
``a``, ``0 <= b < F``, ``b != a`` a surface over ``(a, b)``.

    curve  (a)    [p]    = sum_g sum_t s[g][t] * w_g( x0 with x[a] = u[p]              , pp_g[t] )
    surface(a, b) [p][q] = sum_g sum_t s[g][t] * w_g( x0 with x[a] = u[p], x[b] = u[q] , pp_g[t] )

``w_g`` is the raw SDF tower output in evaluation mode. Every period of the split contributes,
whether or not it has valid stocks (it has a macro state either way); a period whose scale is zero
for all models contributes nothing.

Scales:
  ``"raw"``       ``s = 1 / (G * T_used)``: the plain average raw weight of a hypothetical stock;
  ``"ensemble"``  ``s[g][t] = 1 / (G * T_used * sum_i |wn_g,t,i|)``, ``wn`` the model's (zero-mean)
                  weights as in ``analysis.importance``; zero for a period without a valid row (its
                  L1 norm is zero and is not clamped into a huge scale). ``T_used`` counts the
                  periods with a non-zero scale. The zero-mean shift is a per-period constant:
                  ``offset = sum_g sum_t s[g][t] * mean_i w_g,t,i`` is reported and not subtracted,
                  so ``curve - offset`` is the averaged L1-normalised weight of that stock.

``period_groups`` (int ``[T]``, -1 = skip, else ``0..NG-1``) gives one result set per group of
periods, e.g. expansion / recession months: a group is a scale table that is zero outside it, with
``T_used`` counted per group. Default: one group of all periods.

Defaults: ``base`` is the per-column median of the split's valid characteristic values, ``grid``
21 evenly spaced points between the pooled 5 % and 95 % quantiles of all of them; every
characteristic gets a curve and there are no surfaces (``pairs`` is a list of ``(a, b)`` or
``"all"``).

``device="cpu"`` evaluates the PyTorch tower on the generated rows (any architecture, mixed
ensembles, ``dtype``). ``device="cuda"`` runs ``csrc/k_wsurf.hip`` through
``Engine.weight_surface``: one launch per group for all models and items, the rows generated in
registers. Mixed-architecture ensembles and shapes the kernel does not cover (the wide layer-0
path) fall back to the CPU path with a printed note.

Out of scope: triple interactions, curves over the state columns or the macro series, the moment
network, the indirect effect of a stock on the normalisation.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..models import losses as L
from .importance import _state


def _items(F: int, characteristics, pairs):
    cols = list(range(F)) if characteristics is None else [int(c) for c in characteristics]
    if pairs is None:
        prs = []
    elif isinstance(pairs, str):
        if pairs != "all":
            raise ValueError("pairs must be a list of (a, b) or 'all'")
        prs = [(a, b) for i, a in enumerate(cols) for b in cols[i + 1:]]
    else:
        prs = [(int(a), int(b)) for a, b in pairs]
    for c in cols + [c for p in prs for c in p]:
        if c < 0 or c >= F:
            raise ValueError(f"weight_structure: column {c} outside [0, {F})")
    for a, b in prs:
        if a == b:
            raise ValueError("weight_structure: a surface needs two different columns (a == b)")
    if not cols and not prs:
        raise ValueError("weight_structure: no items")
    return cols, prs


def default_grid_base(batch: Dict, points: int = 21):
    """(grid [points], base [F]) from the split's valid characteristic values."""
    feats = batch["individual_features"]
    mask = batch["mask"].bool()
    v = feats[mask].double().cpu().numpy()             # [rows, F]
    if v.shape[0] == 0:
        return np.linspace(-0.5, 0.5, points), np.zeros(feats.shape[-1])
    lo, hi = np.quantile(v, [0.05, 0.95])
    if not hi > lo:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, points), np.median(v, axis=0)


def make_rows(grid: np.ndarray, base: np.ndarray, cols: Sequence[int], prs: Sequence) -> np.ndarray:
    """The generated feature rows [n1 P + n2 P P, F]: curves first, then surfaces with q fastest."""
    P, F = len(grid), len(base)
    out = np.tile(base[None, :], (len(cols) * P + len(prs) * P * P, 1))
    r = 0
    for a in cols:
        out[r:r + P, a] = grid
        r += P
    for a, b in prs:
        out[r:r + P * P, a] = np.repeat(grid, P)
        out[r:r + P * P, b] = np.tile(grid, P)
        r += P * P
    return out


def _tower(model, x):
    net = model.sdf_net
    return net.output_proj(net.fc_layers(x))[:, 0]


def _group_tables(per_model: np.ndarray, nonzero: np.ndarray, groups: np.ndarray, NG: int, G: int):
    """Scale tables [NG][G][T] = per_model / (G * T_used) inside the group, and T_used [NG]."""
    T = per_model.shape[1]
    s = np.zeros((NG, G, T))
    used = np.zeros(NG, dtype=np.int64)
    for k in range(NG):
        sel = (groups == k) & nonzero
        used[k] = int(sel.sum())
        if used[k]:
            s[k][:, sel] = per_model[:, sel] / (G * used[k])
    return s, used


def _cpu_scale_parts(ms, batch, dtype, scale: str):
    """per_model [G][T] (1, or 1 / L1 norm), nonzero [T] and mean_raw [G][T] (the zero-mean shift)."""
    mask = batch["mask"].bool()
    T = mask.shape[0]
    G = len(ms)
    if scale == "raw":
        return np.ones((G, T)), np.ones(T, dtype=bool), np.zeros((G, T))
    feats = batch["individual_features"].to(dtype)
    macro = batch.get("macro_features")
    macro = None if macro is None else macro.to(dtype)
    mk = mask.to(dtype)
    inv = np.zeros((G, T)); mean = np.zeros((G, T))
    nonzero = mask.any(1).numpy().copy()
    for g, m in enumerate(ms):
        net = m.sdf_net
        st = _state(m, macro)
        with torch.no_grad():
            x = feats if st is None else torch.cat([feats, st[:, None, :].expand(T, feats.shape[1], st.shape[-1])], -1)
            w_raw = _tower(m, x.reshape(T * feats.shape[1], -1)).reshape(T, -1)
        if net.normalize_weights:
            wn = L.zero_mean_normalize(w_raw, mask).to(dtype)
            mean[g] = ((w_raw * mk).sum(1) / mk.sum(1).clamp(min=1)).double().numpy()
        else:
            wn = w_raw * mk
        l1 = (wn.abs() * mk).sum(1).double().numpy()
        nonzero &= l1 > 0
        inv[g] = 1.0 / np.where(l1 > 0, l1, 1.0)
    return inv, nonzero, mean


def _cpu_values(ms, batch, dtype, rows_np: np.ndarray, tables: np.ndarray, chunk: int = 8) -> np.ndarray:
    """values [NG][rows] (float64) of the torch towers on the generated rows."""
    macro = batch.get("macro_features")
    macro = None if macro is None else macro.to(dtype)
    T = int(batch["mask"].shape[0])
    X = torch.as_tensor(rows_np).to(dtype)
    R = X.shape[0]
    NG = tables.shape[0]
    out = np.zeros((NG, R))
    live = np.abs(tables).sum((0, 1)) > 0
    for g, m in enumerate(ms):
        st = _state(m, macro)
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            if not live[t0:t1].any():
                continue
            with torch.no_grad():
                if st is None:
                    w = _tower(m, X)[None].expand(t1 - t0, R)
                else:
                    x = torch.cat([X[None].expand(t1 - t0, R, X.shape[1]),
                                   st[t0:t1, None, :].expand(t1 - t0, R, st.shape[-1])], -1)
                    w = _tower(m, x.reshape((t1 - t0) * R, -1)).reshape(t1 - t0, R)
            out += tables[:, g, t0:t1] @ w.double().numpy()
    return out


def _gpu_values(models, batch, scale: str, grid, base, cols, prs, groups, NG, precision: str):
    """(values [NG][rows], used [NG], offset [NG]) from the native engine, or None (with a printed
    note) where it does not apply."""
    if len({m.spec for m in models}) != 1:
        print("[weight_structure] mixed-architecture ensemble: using the CPU path")
        return None
    from ..engine.runner import GANEngine
    G = len(models)
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = GANEngine(models[0].spec, G, max_epochs=4, precision=precision)
    eng.set_data(batch)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    e = eng.eng
    mask = batch["mask"].bool().cpu().numpy()
    T, N = mask.shape
    try:
        if not e.weight_surface_supported(0):
            print("[weight_structure] weight_surface: not available for this shape: using the CPU path")
            return None
        if scale == "raw":
            inv, nonzero, mean = np.ones((G, T)), np.ones(T, dtype=bool), np.zeros((G, T))
            refresh = True
        else:
            e.forward_split(0, False, False)
            nonzero = mask.any(1)
            inv = np.zeros((G, T)); mean = np.zeros((G, T))
            for g in range(G):
                wn = np.asarray(e.read_ws(g, 0, "wn"), dtype=np.float64)[:T * N].reshape(T, N)
                l1 = (np.abs(wn) * mask).sum(1)
                nonzero = nonzero & (l1 > 0)
                inv[g] = 1.0 / np.where(l1 > 0, l1, 1.0)
                if models[g].sdf_net.normalize_weights:
                    mean[g] = np.asarray(e.read_ws(g, 0, "mu"), dtype=np.float64)[:T]
            refresh = False
        tables, used = _group_tables(inv, nonzero, groups, NG, G)
        items = [(a, -1) for a in cols] + list(prs)
        g32 = [float(x) for x in np.asarray(grid, dtype=np.float32)]
        b32 = [float(x) for x in np.asarray(base, dtype=np.float32)]
        vals = []
        try:
            for k in range(NG):
                sc = torch.as_tensor(tables[k], dtype=torch.float32).to(dev).contiguous()
                torch.cuda.synchronize(dev)
                r = e.weight_surface(0, sc.data_ptr(), g32, b32, items, refresh)
                refresh = False
                vals.append(np.asarray(r["values"], dtype=np.float64))
        except ValueError as err:
            print(f"[weight_structure] {err}: using the CPU path")
            return None
    finally:
        e.sync()
    offset = (tables * np.where(nonzero, mean, 0.0)[None]).sum((1, 2))
    return np.stack(vals), used, offset


def weight_structure(models: Sequence, batch: Dict, device: str = "cpu", scale: str = "ensemble",
                     grid=None, base=None, characteristics=None, pairs=None, period_groups=None,
                     names: Optional[Sequence] = None, precision: str = "bf16",
                     dtype: torch.dtype = torch.float32) -> Dict:
    """Response curves and interaction surfaces of the ensemble SDF weight over ``batch`` (module
    docstring). Returns ``grid`` [P], ``base`` [F], ``names``, ``curve_items`` [n1], ``curves``
    [NG][n1][P], ``pair_items`` [n2] of (a, b), ``surfaces`` [NG][n2][P][P], ``offset`` [NG],
    ``periods_used`` [NG] and ``interaction`` [NG][n2] = max |surface - (curve_a[p] + curve_b[q] -
    curve_mid)|, the departure from additivity (NaN where a curve of the pair is missing;
    ``curve_mid`` is the additive model's value at the base row, taken from the curves and ``base``
    by linear interpolation). ``precision`` applies to the engine, ``dtype`` to the CPU path."""
    if scale not in ("ensemble", "raw"):
        raise ValueError("scale must be 'ensemble' or 'raw'")
    models = list(models)
    if not models:
        raise ValueError("no models")
    feats = batch["individual_features"]
    T, N, F = feats.shape
    cols, prs = _items(F, characteristics, pairs)
    if grid is None or base is None:
        dg, db = default_grid_base(batch)
        grid = dg if grid is None else grid
        base = db if base is None else base
    grid = np.asarray(grid, dtype=np.float64).ravel()
    base = np.asarray(base, dtype=np.float64).ravel()
    if len(grid) < 2 or len(grid) > 64:
        raise ValueError("weight_structure: the grid must have 2 .. 64 points")
    if len(base) != F:
        raise ValueError(f"weight_structure: base must have F = {F} entries")
    if period_groups is None:
        groups = np.zeros(T, dtype=np.int64)
    else:
        groups = np.asarray(period_groups, dtype=np.int64).ravel()
        if len(groups) != T or groups.min() < -1:
            raise ValueError("weight_structure: period_groups must be [T] with values -1 or 0..NG-1")
    NG = max(int(groups.max()) + 1, 1)
    P, n1, n2 = len(grid), len(cols), len(prs)
    r = None
    if str(device).startswith("cuda"):
        r = _gpu_values(models, batch, scale, grid, base, cols, prs, groups, NG, precision)
    if r is None:
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        ms = [copy.deepcopy(m).cpu().to(dtype).eval() for m in models]
        inv, nonzero, mean = _cpu_scale_parts(ms, cpu, dtype, scale)
        tables, used = _group_tables(inv, nonzero, groups, NG, len(ms))
        vals = _cpu_values(ms, cpu, dtype, make_rows(grid, base, cols, prs), tables)
        offset = (tables * np.where(nonzero, mean, 0.0)[None]).sum((1, 2))
        r = (vals, used, offset)
    vals, used, offset = r
    curves = vals[:, :n1 * P].reshape(NG, n1, P)
    surfaces = vals[:, n1 * P:].reshape(NG, n2, P, P)
    inter = np.full((NG, n2), np.nan)
    pos = {c: i for i, c in enumerate(cols)}
    for j, (a, b) in enumerate(prs):
        if a in pos and b in pos:
            ca, cb = curves[:, pos[a]], curves[:, pos[b]]                  # [NG][P]
            for k in range(NG):
                mid = 0.5 * (np.interp(base[a], grid, ca[k]) + np.interp(base[b], grid, cb[k]))
                inter[k, j] = np.abs(surfaces[k, j] - (ca[k][:, None] + cb[k][None, :] - mid)).max()
    nm = [str(n) for n in names] if names is not None and len(names) == F else [f"x{j}" for j in range(F)]
    return {"grid": grid, "base": base, "names": nm, "curve_items": list(cols), "curves": curves,
            "pair_items": [tuple(p) for p in prs], "surfaces": surfaces, "offset": np.asarray(offset),
            "periods_used": np.asarray(used), "interaction": inter, "scale": scale}


def parse_pairs(spec, names: Optional[Sequence] = None):
    """CLI form of ``pairs``: None, ``"all"`` or a comma list of ``A:B`` by name or column index."""
    if spec is None or spec == "" or spec == "all":
        return spec or None
    if not isinstance(spec, str):
        return spec
    idx = {str(n): i for i, n in enumerate(names)} if names is not None else {}

    def col(tok):
        tok = tok.strip()
        if tok in idx:
            return idx[tok]
        try:
            return int(tok)
        except ValueError:
            raise ValueError(f"structure_pairs: unknown characteristic {tok!r}") from None
    out = []
    for item in spec.split(","):
        ab = item.split(":")
        if len(ab) != 2:
            raise ValueError(f"structure_pairs: expected A:B, got {item!r}")
        out.append((col(ab[0]), col(ab[1])))
    return out


def format_structure(ws: Dict, top: int = 12) -> List[str]:
    """The printed report: per group the characteristics with the largest curve range (and its
    direction), then the pairs with the largest departure from additivity."""
    lines = []
    names, grid = ws["names"], ws["grid"]
    for k in range(ws["curves"].shape[0]):
        lines.append(f"  Group {k}: {int(ws['periods_used'][k])} periods, offset {ws['offset'][k]:+.4e}, "
                     f"grid [{grid[0]:+.3f}, {grid[-1]:+.3f}] x {len(grid)}")
        c = ws["curves"][k]
        if len(c):
            rng = c.max(1) - c.min(1)
            for i, j in enumerate(np.argsort(-rng)[:top]):
                slope = c[j, -1] - c[j, 0]
                lines.append(f"    {i + 1:2d}. {names[ws['curve_items'][j]]:<16s} range {rng[j]:.4e}  end-to-end {slope:+.4e}")
        it = ws["interaction"][k]
        if len(it):
            lines.append("    Departure from additivity (max |surface - additive|):")
            order = np.argsort(-np.nan_to_num(it, nan=-1.0))[:top]
            for j in order:
                a, b = ws["pair_items"][j]
                lines.append(f"        {names[a]:<16s} x {names[b]:<16s} {it[j]:.4e}")
    return lines


def to_json(ws: Dict) -> Dict:
    out = {}
    for k, v in ws.items():
        if isinstance(v, np.ndarray):
            out[k] = v.tolist()
        elif k == "pair_items":
            out[k] = [list(p) for p in v]
        else:
            out[k] = v
    return out
