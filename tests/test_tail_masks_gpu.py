"""Next-step dropout keep words from blocks of the backward tail launch (``DLAP_TAIL_MASKS``), on a
real MI355X.

With the split epoch graphs the tail launch of an epoch (``k_lstm_tail``) carries mask blocks that
hash the keep words of dropout step ``drop_step + 1`` -- ``k_dropmask``'s body, the same words at
the same addresses -- and the evaluation graph launches no ``k_dropmask``. ``DLAP_TAIL_MASKS=0`` is
the comparison path: every bit of a run (history rows, parameters, the keep words themselves) must
be equal with the switch on and off.

The plan turns the mask blocks on for one model per engine only (batched launches measured slower
with them, ``profiles/fwd_bptt_tail_masks_bench.txt``); ``DLAP_TAIL_MASKS=N`` (N > 1) forces N mask
blocks per model at any batch size, which is how the three-model cases run the two-waves-per-SIMD
build of the tail with mask blocks. In every on-arm the path must be active (asserted, no skip).

Panel sizes: the split graphs need the fused training forward, which the plan grants only from 16
tower workgroups of 4 tiles (61 tiles, 1921 rows) upwards. The stock count of a case is therefore
the smallest that leaves about 2000 rows in its ``T - 1`` non-empty periods, not the ~40 stocks a
panel without that floor could use: at 40 stocks the paths under test never run. One period is
fully masked and the row count is no multiple of 32 (asserted)."""
import itertools

import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

F = 46
ROWS = 2000                                      # about this many rows: 63 tiles, 16 tower workgroups
FORCED_BLOCKS = 7                                # batched on-arm: 7 blocks of 10-11 tiles, the last one short
SCHEDULE = ((1, 1), (1, 2), (1, 10), (2, 2), (3, 10))   # head only | one body | unrolled + single bodies


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


_PANELS = {}


def _panel(T, M):
    """T periods (period 1 fully masked), M macro series, a row count that is no multiple of 32."""
    if (T, M) not in _PANELS:
        N = -(-ROWS // (T - 1)) + 37
        ret, feats, mask, mac = generate_panel_fast(T, N, F, M, seed=T)
        mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
        mask = mask.clone()
        mask[1] = False
        if int(mask.sum()) % 32 == 0:
            t, i = torch.nonzero(mask)[0].tolist()
            mask[t, i] = False
        _PANELS[(T, M)] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[(T, M)]


def _engine(monkeypatch, on, T, M, hidden, dropout, G, blocks=FORCED_BLOCKS):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    # one model: the plan's own choice; batched models: forced (`blocks` mask blocks per model)
    monkeypatch.setenv("DLAP_TAIL_MASKS", ("1" if G == 1 else str(blocks)) if on else "0")
    cfg = default_cli_config(M, F, hidden_dim=list(hidden), rnn_dim=[4], dropout=dropout)
    b = _panel(T, M)
    R = int(b["mask"].sum())
    assert R % 32 != 0 and not bool(b["mask"][1].any())
    eng = GANEngine(AssetPricingGAN(cfg).spec, G, max_epochs=32)
    eng.set_data(b, b, b)
    for g in range(G):
        torch.manual_seed(500 + g)
        eng.set_model(g, AssetPricingGAN(cfg), 21 + g)
    info = eng.eng.fused_info()
    assert info["split_graphs"] and info["fused_tail"], info
    # the path under test is active in the on-arm (dropout 0 has no keep words: no mask blocks)
    assert bool(info["tail_masks"]) == (on and dropout > 0), info
    if info["tail_masks"]:
        # more than one block: one model, ranges of at most 16 tiles (one pass of a block's four waves)
        nb, ntiles = info["tail_mask_blocks"], (R + 31) // 32
        assert nb == (blocks if G > 1 else (ntiles + 15) // 16) and nb >= 2, (info, ntiles)
    return eng


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _run(monkeypatch, on, case):
    T, M, hidden, dropout, G = case
    eng = _engine(monkeypatch, on, T, M, hidden, dropout, G)
    for ph, n in SCHEDULE:
        eng.eng.begin_phase(ph)
        eng.run(ph, n, 1e-3, 1, 1.0, True)
    eng.eng.sync()
    assert eng.eng.prog_timeouts() == 0
    out = []
    for g in range(G):
        hist = eng.history_rows(g)
        assert hist.shape[0] == sum(n for _, n in SCHEDULE)
        out.append((_bits(hist), _bits(eng.params(g)), _bits(eng.params(g, "loss")), _bits(eng.params(g, "sharpe")),
                    eng.eng.get_opt_state(g)["drop_step"]))
    return out


CASES = list(itertools.product((2, 3, 9, 17), (3, 17), ((8,), (8, 8), (8, 8, 8)), (0.0, 0.05, 0.5), (1, 3)))


def _case_id(c):
    T, M, hidden, dropout, G = c
    return f"T{T}-M{M}-h{len(hidden)}-d{dropout:g}-G{G}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_tail_masks_equal_k_dropmask_on_the_eval_queue(monkeypatch, case):
    """History rows, parameters and snapshots bitwise equal with the mask blocks on and off, over the
    head, one-body, unrolled-body and tail graphs of phase 1, a phase 2 in between and phase 3."""
    ref = _run(monkeypatch, False, case)
    res = _run(monkeypatch, True, case)
    for a, b in zip(ref, res):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_batched_models_keep_k_dropmask_by_default(monkeypatch):
    """The plan's choice by batch size: at the default switch position a three-model engine runs the
    split graphs without mask blocks; safe mode turns the path off for one model too."""
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    monkeypatch.setenv("DLAP_TAIL_MASKS", "1")
    cfg = default_cli_config(3, F, hidden_dim=[8, 8], rnn_dim=[4], dropout=0.05)
    b = _panel(9, 3)
    for G in (1, 3):
        eng = GANEngine(AssetPricingGAN(cfg).spec, G, max_epochs=8)
        eng.set_data(b, b, b)
        for g in range(G):
            torch.manual_seed(500 + g)
            eng.set_model(g, AssetPricingGAN(cfg), 21 + g)
        info = eng.eng.fused_info()
        assert info["split_graphs"] and bool(info["tail_masks"]) == (G == 1), info
        assert (info["tail_mask_blocks"] > 0) == (G == 1), info
        eng.eng.set_safe_mode(True)
        info = eng.eng.fused_info()
        assert not info["split_graphs"] and not info["tail_masks"] and info["tail_mask_blocks"] == 0, info


@pytest.mark.parametrize("G", (1, 3))
def test_tail_mask_words_equal_k_dropmask_words(monkeypatch, G):
    """After head + two body epochs both parity halves were last written by a body epoch: by the
    tail's mask blocks in the on-arm, by k_dropmask in the off-arm. Same words, both halves."""
    words = {}
    for on in (False, True):
        # (three models: 2 blocks of 36 tiles, three passes per wave, the last one partial)
        eng = _engine(monkeypatch, on, 9, 3, (8, 8), 0.5, G, blocks=2)
        eng.eng.begin_phase(1)
        eng.run(1, 3, 1e-3, 1, 1.0, True)
        eng.eng.sync()
        assert eng.eng.prog_timeouts() == 0
        words[on] = [(eng.eng.get_opt_state(g)["drop_step"], eng.eng.keep_words(g, 0), eng.eng.keep_words(g, 1))
                     for g in range(G)]
    for (s0, a0, a1), (s1, b0, b1) in zip(words[False], words[True]):
        assert s0 == s1
        np.testing.assert_array_equal(a0, b0)
        np.testing.assert_array_equal(a1, b1)
        # the halves hold two different steps' words, at rate 0.5 about half the bits set
        assert not np.array_equal(b0, b1)
        for w in (b0, b1):
            frac = np.unpackbits(w.view(np.uint8)).mean()
            assert 0.45 < frac < 0.55, frac
