"""Shared cases of the tree-pruning tests: planted factor returns, their moments from
``tree_prune.mv_moments`` and a few penalty paths; the numpy oracle of a case is computed once."""
import functools

import numpy as np

from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp

MAX_SWEEPS = 200          # of every case: keeps an oracle at about 2 s on the CPU at most

# name -> (n, T, seed, ((l0, l2_rel), ..) per path, n1, decades of l1, max_assets, zero-diagonal coordinates)
_THREE = ((0.0, 1e-2), (0.25, 1e-1), (0.5, 1e-3))
CASES = {
    "n1": (1, 12, 1, _THREE, 6, 3.0, None, ()),
    "n13": (13, 40, 2, _THREE, 8, 3.0, None, ()),
    "n64": (64, 150, 3, _THREE, 8, 3.0, None, ()),
    "n70": (70, 150, 4, _THREE, 8, 3.0, None, ()),
    "n257": (257, 500, 5, _THREE, 5, 1.5, None, ()),
    "n300": (300, 600, 6, _THREE, 5, 1.25, None, ()),
    "rank_deficient": (70, 30, 7, ((0.0, 0.0), (0.25, 0.0)), 6, 3.0, None, ()),      # l2 = 0, T < n: the cap is hit
    "zero_diagonal": (40, 60, 8, ((0.25, 0.0), (0.25, 1e-2)), 6, 3.0, None, (0, 17, 39)),
    "max_assets": (70, 60, 9, _THREE, 10, 3.0, 5, ()),
    # one case per row-buffer size of the kernel above the listed ones (4, 8, 16 elements a thread at 256
    # threads, the last at ENCD_MAX_N); sparse and short, so the oracle stays quick
    "n600": (600, 50, 12, _THREE[:2], 4, 1.0, 4, ()),
    "n1100": (1100, 50, 13, _THREE[:2], 4, 1.0, 4, ()),
    "n2100": (2100, 40, 14, _THREE[:2], 4, 0.3, 12, ()),
    "n4096": (4096, 32, 15, _THREE[:2], 4, 0.2, 12, ()),
}


def planted_returns(T: int, n: int, seed: int, K: int = 4) -> np.ndarray:
    """Returns [T][n] of ``n`` assets that load on ``K`` priced factors, plus noise."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, K)) * 0.02
    f = rng.standard_normal((T, K)) + 0.3
    return f @ B.T + 0.05 * rng.standard_normal((T, n))


def paths_of(mu, S, pens, n1, decades):
    n = mu.shape[0]
    b = np.array([mu + l0 * mu.mean() for l0, _ in pens])
    l2 = np.array([r2 * np.trace(S) / n for _, r2 in pens])
    l1s = np.array([np.abs(bp).max() * 10.0 ** (-np.linspace(0.0, decades, n1)) for bp in b])
    return b, l1s, l2


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    n, T, seed, pens, n1, decades, max_assets, zero_diag = CASES[name]
    R = planted_returns(T, n, seed)
    for j in zero_diag:
        R[:, j] = 0.0                                  # a column of zeros: S[j][:] = S[:][j] = 0, diag = l2
    mu, S = tp.mv_moments(R)
    b, l1s, l2 = paths_of(mu, S, pens, n1, decades)
    return {"A": S[None].copy(), "a_of": np.zeros(len(pens), np.int32), "b": b, "l1s": l1s, "l2": l2,
            "max_sweeps": MAX_SWEEPS, "max_assets": max_assets, "zero_diag": zero_diag}


@functools.lru_cache(maxsize=None)
def two_matrix_case() -> dict:
    """Four paths over two matrices (different periods of one panel), interleaved through ``a_of``."""
    n = 45
    R = planted_returns(100, n, 10)
    (mu0, S0), (mu1, S1) = tp.mv_moments(R[:50]), tp.mv_moments(R[50:])
    a_of = np.array([1, 0, 0, 1], np.int32)
    pens = ((0.0, 1e-2), (0.0, 1e-2), (0.5, 1e-1), (0.25, 1e-3))
    b, l1s, l2 = [], [], []
    for a, pen in zip(a_of, pens):
        bb, ll, l = paths_of((mu0, mu1)[a], (S0, S1)[a], (pen,), 6, 3.0)
        b.append(bb[0]); l1s.append(ll[0]); l2.append(l[0])
    return {"A": np.stack([S0, S1]), "a_of": a_of, "b": np.array(b), "l1s": np.array(l1s), "l2": np.array(l2),
            "max_sweeps": MAX_SWEEPS, "max_assets": None, "zero_diag": ()}


def call_args(c: dict) -> tuple:
    return c["A"], c["a_of"], c["b"], c["l1s"], c["l2"]


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> dict:
    c = two_matrix_case() if name == "two_matrices" else case(name)
    return tp.en_paths_numpy(*call_args(c), max_sweeps=c["max_sweeps"], max_assets=c["max_assets"])


# ---- a small planted panel for prune_trees: 2 keys, depth 2, 40 / 20 / 20 periods ---------------------
@functools.lru_cache(maxsize=None)
def planted_panel() -> dict:
    """``tree_sorts.tree_sort_numpy`` inputs per split: the return loads on the two keys, so the tree
    nodes carry different mean returns."""
    rng = np.random.default_rng(11)
    N = 60
    out = {}
    for s, T in (("train", 40), ("valid", 20), ("test", 20)):
        keys = rng.uniform(-0.5, 0.5, (T, N, 2)).astype(np.float32)
        mask = rng.uniform(size=(T, N)) < 0.9
        f = 0.02 + 0.05 * rng.standard_normal((T, 1))
        ret = (f * (1.0 + keys[:, :, 0]) + 0.04 * keys[:, :, 1] + 0.05 * rng.standard_normal((T, N))).astype(np.float32)
        out[s] = {"keys": keys, "mask": mask, "returns": ret}
    return out


@functools.lru_cache(maxsize=None)
def planted_tree_results() -> dict:
    """The shape of ``tree_sorted_portfolios``' result (the keys ``prune_trees`` reads) per split, from
    the numpy definition of the sort."""
    from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
    trees, splits = ts.all_trees([0, 1], 2), (2, 2)
    out = {}
    for s, d in planted_panel().items():
        vals = np.stack([d["returns"], np.zeros_like(d["returns"])], axis=2)
        raw = ts.tree_sort_numpy(d["keys"], trees, d["mask"], vals, splits)
        cnt = raw["count"]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(cnt[..., None] > 0, raw["sum"] / cnt[..., None], np.nan)
        out[s] = {"returns": mean[..., 0], "count": cnt, "trees": [tuple(t) for t in trees], "splits": splits,
                  "names": [" > ".join(str(c) for c in t) for t in trees], "level_offsets": raw["level_offsets"]}
    return out
