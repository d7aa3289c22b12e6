"""Synthetic generator: the reference-stream generator reproduces the shipped files bit-for-bit
(recorded digests of the reference's ``data/synthetic_data``, ``tests/golden/shipped_data.json``);
the fast torch generator produces the same schema/statistics at scale."""
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from deeplearninginassetpricing_paperreplication_amd.data import synthetic as syn


def test_generate_all_splits_reproduces_shipped_data(tmp_path):
    syn.generate_all_splits(str(tmp_path), 120, 30, 60, n_stocks=500, n_features=46, n_macro=8, seed=42,
                            quiet=True)
    shipped = gc.load_json("shipped_data.json")
    for sub, name in gc.SHIPPED_FILES:
        a = shipped[f"{sub}/{name}"]
        with np.load(tmp_path / sub / name, allow_pickle=False) as b:
            assert a["files"] == b.files, name
            for k in a["files"]:
                assert a["arrays"][k]["dtype"] == str(b[k].dtype), (name, k)
                assert a["arrays"][k]["digest"] == gc.digest(b[k]), f"{name}:{k}"


def test_public_building_blocks_match_reference():
    ref = gc.load_npz("synthetic_blocks.npz")
    fa, ba, ca, ra, ma, ka = (ref[k] for k in ("factor_returns", "factor_loadings", "characteristics",
                                               "returns", "macro", "missing"))
    np.random.seed(7)
    fb = syn.generate_factor_returns(30, 5)
    bb = syn.generate_factor_loadings(40, 5)
    cb = syn.generate_characteristics(30, 40, 12, bb)
    rb = syn.generate_returns(fb, bb)
    mb = syn.generate_macro_features(30, 8, fb)
    kb = syn.generate_missing_pattern(30, 40)
    for x, y in ((fa, fb), (ba, bb), (ra, rb), (ma, mb), (ka, kb)):
        assert x.dtype == np.asarray(y).dtype
        np.testing.assert_array_equal(x, y)
    np.testing.assert_allclose(cb, ca, rtol=1e-12, atol=1e-12)
    d = np.random.RandomState(0).randn(5, 6, 3)
    m = np.random.RandomState(1).rand(5, 6) > 0.5
    np.testing.assert_array_equal(syn.apply_missing_values(d, m), ref["apply_missing_values"])
    ia = {k[len("individual_npz/"):]: v for k, v in ref.items() if k.startswith("individual_npz/")}
    ib = syn.create_individual_npz(rb, cb, kb, 12, 196703)
    assert set(ia) == set(ib)
    for k in ia:
        assert np.array_equal(ia[k], ib[k]) or np.allclose(ia[k], ib[k], atol=1e-6), k


def test_split_date_quirk():
    assert syn.split_start_dates(120, 30) == (196703, 198703, 199203)


def test_generate_panel_fast_shapes_and_stats():
    ret, feats, mask, mac = syn.generate_panel_fast(36, 300, 20, 6, seed=3)
    assert ret.shape == (36, 300) and feats.shape == (36, 300, 20) and mask.shape == (36, 300)
    assert mac.shape == (36, 6) and feats.dtype == torch.float32 and mask.dtype == torch.bool
    cov = mask.float().mean().item()
    assert 0.3 < cov < 0.95
    m = mask[:, :, None].expand_as(feats)
    f = feats[m]
    assert abs(f.mean().item()) < 0.1 and 0.7 < f.std().item() < 1.3
    r2, f2, k2, m2 = syn.generate_panel_fast(36, 300, 20, 6, seed=3)
    assert torch.equal(ret, r2) and torch.equal(mask, k2)      # deterministic per seed
