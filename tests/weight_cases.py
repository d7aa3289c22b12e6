"""Shared cases of the tree-weight tests: a small panel with the edge cases of the tree sort, the plain
per-row loop of the definition, coefficient tables, and the planted panel of ``prune_cases`` as batches
with a pruned SDF on it. Every sort and oracle is computed once."""
import functools

import numpy as np
import torch

import prune_cases as pc
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts

SMALL_SPLITS = [(2, 2, 2), (3, 4), (2, 2, 2, 2, 2)]


@functools.lru_cache(maxsize=None)
def small_panel():
    """keys [6][40][5], mask, returns: masked stocks, an empty period (3), a period of 5 rows (1: fewer than
    the 8, 12 and 32 leaves), a constant key (0) and a key with both signed zeros (2)."""
    rng = np.random.default_rng(5)
    T, N, F = 6, 40, 5
    keys = rng.standard_normal((T, N, F)).astype(np.float32)
    keys[:, :, 0] = 0.375
    z = np.arange(N) % 5
    keys[:, z == 0, 2] = -0.0
    keys[:, z == 1, 2] = 0.0
    mask = rng.uniform(size=(T, N)) < 0.9
    mask[:, np.arange(N) % 7 == 3] = False
    mask[3] = False
    mask[1] = False
    mask[1, [2, 9, 18, 30, 33]] = True
    ret = (0.05 * rng.standard_normal((T, N))).astype(np.float32)
    assert int(mask[1].sum()) == 5 and np.signbit(keys[:, :, 2]).any() and (keys[:, :, 2] == 0).any()
    return keys, mask, ret


def small_trees(D: int):
    """The rotations of the five keys, a repeated key at every level and the signed-zero key twice."""
    out = [tuple((s + k) % 5 for k in range(D)) for s in range(5)]
    return out + [(1,) * D, tuple((2, 2, 4, 1, 3)[:D])]


@functools.lru_cache(maxsize=None)
def small_sort(splits: tuple):
    """trees and ``tree_sort_numpy``'s result (values: the return) of the small panel."""
    keys, mask, ret = small_panel()
    trees = small_trees(len(splits))
    return trees, ts.tree_sort_numpy(keys, trees, mask, ret[:, :, None], splits)


def dense_coef(P: int, NN: int, seed: int, decades: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((P, NN))
    if decades:
        c = c * 10.0 ** rng.integers(-decades, decades + 1, (P, NN))
    assert (c != 0).all()
    return c


def sparse_coef(P: int, splits) -> np.ndarray:
    """3 non-zero nodes on 2 trees, one of them a root."""
    lay = ts.tree_layout(splits)
    off = lay["level_offsets"]
    c = np.zeros((P, lay["nodes"]), np.float64)
    c[1, 0] = 0.75                                   # the root of tree 1
    c[1, off[1] + 1] = -1.25                         # child 1 of its level 1
    c[P - 2, off[lay["depth"]] + 2] = 3.0            # a leaf of another tree
    return c


def one_hot_leaves(P: int, splits, p: int) -> np.ndarray:
    lay = ts.tree_layout(splits)
    c = np.zeros((P, lay["nodes"]), np.float64)
    c[p, lay["level_offsets"][lay["depth"]]:] = 1.0
    return c


def loop_weights(keys, trees, mask, splits, breaks, count, coef) -> np.ndarray:
    """The definition row by row in Python floats: the float64 ``acc`` [T][N] (0 at the invalid cells)."""
    lay = ts.tree_layout(splits)
    qs, D, off, boff = lay["splits"], lay["depth"], lay["level_offsets"], lay["break_offsets"]
    T, N, _ = keys.shape
    out = np.zeros((T, N), np.float64)
    for t in range(T):
        for i in range(N):
            if not mask[t, i]:
                continue
            acc = 0.0
            for p, tr in enumerate(trees):
                node = 0
                for l in range(D + 1):
                    if l >= 1:
                        Q = qs[l - 1]
                        key = keys[t, i, tr[l - 1]] + keys.dtype.type(0)
                        q = 0
                        for d in range(Q - 1):
                            if key > breaks[t, p, boff[l - 1] + node * (Q - 1) + d]:
                                q += 1
                        node = node * Q + q
                    c = float(coef[p, off[l] + node])
                    if c != 0:
                        acc = acc + c / float(count[t, p, off[l] + node])
            out[t, i] = acc
    return out


def bits32(x) -> np.ndarray:
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)


def bits64(x) -> np.ndarray:
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float64
    return x.view(np.uint64)


def node_sum_bound(n, absum, ref):
    """The bound of the node sums of ``test_tree_sorts_gpu``: two float64 sums of the same ``n`` products in
    another order differ by at most ``n 2^-52 sum |v|``, plus one ulp of the result."""
    return np.asarray(n, dtype=np.float64) * 2.0 ** -52 * absum + np.spacing(np.abs(ref))


# ---- the planted panel of prune_cases as batches, its sorts with their breakpoints, a pruned SDF ------
@functools.lru_cache(maxsize=None)
def planted_case():
    """``(pr, res_by_split, batches)``: ``prune_cases.planted_tree_results()`` plus the ``breaks`` of the same
    sorts, the panel as the batches the analysis functions take (8 macro series for an engine) and
    ``prune_trees`` on it."""
    trees, splits = ts.all_trees([0, 1], 2), (2, 2)
    rng = np.random.default_rng(3)
    by_split, batches = {}, {}
    for s, d in pc.planted_panel().items():
        vals = np.stack([d["returns"], np.zeros_like(d["returns"])], axis=2)
        raw = ts.tree_sort_numpy(d["keys"], trees, d["mask"], vals, splits)
        res = dict(pc.planted_tree_results()[s])
        assert np.array_equal(res["count"], raw["count"])
        res["breaks"], res["break_offsets"] = raw["breaks"], raw["break_offsets"]
        by_split[s] = res
        T = d["mask"].shape[0]
        batches[s] = {"returns": torch.from_numpy(d["returns"]), "individual_features": torch.from_numpy(d["keys"]),
                      "mask": torch.from_numpy(d["mask"]),
                      "macro_features": torch.from_numpy(rng.standard_normal((T, 8)).astype(np.float32))}
    pr = tp.prune_trees(by_split, n1=8, max_assets=6, max_sweeps=pc.MAX_SWEEPS, device="cpu")
    return pr, by_split, batches


# ---- the panels of the GPU tests (built like those of test_tree_sorts_gpu) ------------------------------
KEYS_A = [0, 3, 1, 2, 4, 7, 45]
KEYS_B = [1, 5, 6, 2]                  # 5, 6: the extra keys
_PANELS = {}


def gpu_trees(keys, D, count):
    """``count`` trees of depth D on ``keys``: the rotations (every key at every level), then a repeated key,
    then mixed ones."""
    n = len(keys)
    out = [tuple(keys[(s + k) % n] for k in range(D)) for s in range(n)]
    out += [(keys[1],) * D, tuple(keys[(2 * k) % n] for k in range(D)), tuple(keys[-1 - k % 2] for k in range(D))]
    return out[:count]


def gpu_panel(name):
    """``(batch, extra keys [E][T][N] fp32 or None)``. A (12 x 150 x 46): masked stocks, an empty period (5), a
    period of 7 stocks (2), a constant column (0), a column of 4 values (1), a column with both signed zeros
    (2). B (3 x 2600 x 5): eleven row segments per period, an extra key that only the lowest mantissa bit
    separates and one of both signs over many decades. W (4 x 64 x 130): the wide layer-0 path."""
    from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
    if name in _PANELS:
        return _PANELS[name]
    rng = np.random.default_rng(11)
    if name == "A":
        ret, feats, mask, mac = generate_panel_fast(12, 150, 46, 8, seed=0)
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False
        mask[5] = False
        keep = torch.nonzero(mask[2]).flatten()[::19][:7]
        mask[2] = False
        mask[2, keep] = True
        assert int(mask[2].sum()) == 7
        feats = feats.clone()
        feats[:, :, 0] = 0.375
        feats[:, :, 1] = torch.bucketize(feats[:, :, 1].contiguous(), torch.tensor([-0.5, 0.0, 0.5])).float() - 1.5
        z = torch.arange(150) % 5
        feats[:, z == 0, 2] = -0.0
        feats[:, z == 1, 2] = 0.0
        extra = None
    elif name == "B":
        ret, feats, mask, mac = generate_panel_fast(3, 2600, 5, 8, seed=1)
        perm = np.stack([rng.permutation(2600) for _ in range(3)])
        low = (1.0 + perm.astype(np.float64) * 2.0 ** -23).astype(np.float32)
        both = (rng.standard_normal((3, 2600)) * 10.0 ** rng.integers(-3, 4, (3, 2600))).astype(np.float32)
        assert all(len(np.unique(low[t])) == 2600 and len(np.unique(both[t])) == 2600 for t in range(3))
        extra = np.stack([low, both])
    else:
        ret, feats, mask, mac = generate_panel_fast(4, 64, 130, 8, seed=2)
        mask = mask.clone()
        mask[1, ::3] = False
        extra = None
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    _PANELS[name] = ({"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}, extra)
    return _PANELS[name]


def engine_keys(name, precision) -> np.ndarray:
    """The keys [T][N][F + E] as an engine of ``precision`` holds them: bf16-rounded characteristics for a bf16
    panel, the extra keys in fp32."""
    b, extra = gpu_panel(name)
    f = b["individual_features"]
    keys = (f.to(torch.bfloat16).to(f.dtype) if precision == "bf16" else f).numpy().astype(np.float32)
    if extra is not None:
        keys = np.concatenate([keys, np.moveaxis(extra, 0, 2)], axis=2)
    return keys
