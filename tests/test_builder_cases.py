"""The builder cases of tests/builder_cases.py are what their docstring says, and every condition that
tests/test_gpu_builder_structured.py demands of the kernels holds for the REFERENCE alone (CPU only): the float64
references are finite where a value exists, the kinds have the normaliser products they are named for, the float32
op-by-op restatement's gradients are within 1e-5 of float64 on the sound kinds (a tenth of the GPU tolerance: measured
worst 2.9e-6, `wide` with the occupancies as weights) and return NaN on the unsound ones, and the float32 oracle meets the
forward bound with a factor 2 to spare (measured worst ratio 0.27 of the bound, builder_cases.K_ROUND)."""
import numpy as np
import pytest
import torch

import builder_cases as BC

LOG_TINY = float(np.log(BC.TINY))
_STRICT = {"loose": False, "strict": True}


@pytest.mark.parametrize("strict", list(_STRICT))
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_case_is_what_its_kind_says(kind, shape, strict):
    strict = _STRICT[strict]
    c = BC.make_case(kind, shape, strict)
    B, T, S, C = shape
    am, lm, sym, bd = c["am"], c["lm"], c["symbols"], c["boundary"]
    assert am.dtype == np.float32 and lm.dtype == np.float32 and sym.dtype == np.int32 and bd.dtype == np.int32
    assert am.shape == (B, T, C) and lm.shape == (B, S + 1, C) and sym.shape == (B, S)
    assert not np.isnan(am).any() and not np.isnan(lm).any() and not np.isposinf(am).any() and not np.isposinf(lm).any()
    assert sym.min() >= 0 and sym.max() < c["blank"] and not np.isin(sym, c["free"]).any()
    assert tuple(bd[0]) == (0, 0, min(S, T - 4) if strict and S > T else S, T)          # utterance 0 full size
    for b in range(B):
        se, te = int(bd[b, 2]), int(bd[b, 3])
        ts = c["ts"][b]
        assert 0 < te <= T and 0 < se <= S and len(ts) == se and ts.min() >= 0 and ts.max() < te
        assert (np.diff(ts) >= (1 if strict else 0)).all() and np.bincount(ts).max() <= (1 if strict else 2)
        if b and T % 4 == 0:
            assert te % 4 != 0
        # am peaks on what the path emits (blank where it emits nothing), lm on its target
        emit = np.full(te, c["blank"]); emit[ts[::-1]] = sym[b, :se][::-1]
        if kind not in ("offset", "masked"):
            assert (am[b, :te].argmax(axis=1) == emit).mean() > (0.99 if c["margin"] >= 12 else 0.0)
    if kind == "masked":
        assert np.isneginf(lm[:, :, c["masked_lm"]]).all() and np.isneginf(am[:, :, c["masked_am"]]).all()
        assert np.isfinite(np.delete(lm, c["masked_lm"], axis=2)).all() and np.isfinite(np.delete(am, c["masked_am"], axis=2)).all()
        assert c["blank"] not in c["masked_lm"] and len(c["masked_lm"]) == 3 and c["masked_am"][0] in c["masked_lm"]
    else:
        assert np.isfinite(am).all() and np.isfinite(lm).all()
    p64 = BC.products64(am, lm); p32 = BC.products32(am, lm); v = c["valid"]
    if kind in BC.SOUND:                 # the gradient exists: prod stays a normal float32, on every cell
        assert p64.min() >= BC.F32_MIN_NORMAL and p32.min() >= BC.F32_MIN_NORMAL
    if kind == "wide":
        assert BC.WIDE_INTERVAL[0] <= p64[v].min() <= BC.WIDE_INTERVAL[1], p64[v].min()
        assert 55.0 < c["margin"] < 95.0
    if kind == "offset":
        assert np.abs(am).max() > 250 and np.abs(lm).max() > 350
    if kind == "subnormal":
        share = np.mean((p64[v] >= BC.low_cut(C)) & (p64[v] < BC.F32_MIN_NORMAL))
        assert share >= 0.5, share
    if kind == "zero":
        assert c["margin"] == 120.0 and np.mean(p32[v] == 0.0) >= 0.5


def _oracle_forward(oracle, c, builder, rnnt_type):
    if builder is None:
        return oracle.get_rnnt_logprobs(c["lm"], c["am"], c["symbols"], c["blank"], rnnt_type, c["boundary"])
    return oracle.get_rnnt_logprobs_smoothed(c["lm"], c["am"], c["symbols"], c["blank"], builder[0], builder[1], c["boundary"], rnnt_type)


def _expected_neg_inf(c, rnnt_type):
    """px is -inf in column T and in column t_end of the regular type, and nowhere else; py nowhere."""
    B, T, S = c["B"], c["T"], c["S"]
    pat = np.zeros((B, S, T + 1 if rnnt_type == "regular" else T), bool)
    if rnnt_type == "regular":
        pat[:, :, T] = True
        for b in range(B):
            pat[b, :, int(c["boundary"][b, 3])] = True
    return pat


@pytest.mark.parametrize("rnnt_type", BC.TYPES)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_reference_alone_meets_every_condition(oracle, kind, shape, rnnt_type):
    for builder in BC.BUILDERS:
        ref = BC.reference(oracle, kind, shape, rnnt_type, builder)
        c = ref["case"]
        B, T, S, C = shape
        what = f"{kind} {BC.shape_id(shape)} {rnnt_type} {BC.builder_id(builder)}"
        # float64 reference: finite wherever the lattice has a value, a finite loss for every utterance
        pat = _expected_neg_inf(c, rnnt_type)
        assert np.array_equal(np.isneginf(ref["px"]), pat) and np.isfinite(ref["px"][~pat]).all() and np.isfinite(ref["py"]).all(), what
        assert np.isfinite(ref["ans64"]).all(), what
        # the float32 oracle: same pattern, and the forward bound with a factor 2 to spare
        opx, opy = _oracle_forward(oracle, c, builder, rnnt_type)
        assert np.array_equal(np.isneginf(opx), pat) and np.isfinite(opx[~pat]).all() and np.isfinite(opy).all(), what
        bx, by, low, lowx = BC.forward_bounds(ref, rnnt_type, kind in BC.UNSOUND)
        rx = BC.bound_ratio(opx, ref["px"], bx, lowx); ry = BC.bound_ratio(opy, ref["py"], by, low)
        assert max(rx, ry) <= 0.5, (what, rx, ry)
        if kind in BC.UNSOUND and builder is None:
            # the cells below the cut: a finite value, the normaliser not below log(tiny) + lm_max + am_max
            nrm32 = oracle._normalizers(c["lm"], c["am"])[0]
            floor = LOG_TINY + c["lm"].astype(np.float64).max(axis=2)[:, :, None] + c["am"].astype(np.float64).max(axis=2)[:, None, :]
            assert (nrm32 >= floor - 1e-3).all(), what
            assert low[c["valid"]].mean() <= 0.5 or kind == "zero"       # the exclusion hides at most half of a `subnormal` case
        # the loss the GPU tests ask for (rtol 1e-4 against float64): the float32 oracle's own px / py give it to 2e-5
        l64 = BC.loss64(oracle, ref, rnnt_type, 0.0)
        l32 = -oracle.mutual_information_recursion(opx.astype(np.float64), opy.astype(np.float64), c["boundary"], False, np.float64)
        assert np.isfinite(l64).all() and np.abs(l32 - l64).max() <= 2e-5 * np.abs(l64).max(), (what, l32, l64)
        if kind not in BC.SOUND:
            continue
        if builder not in BC.BWD_BUILDERS:
            continue
        gx64, gy64 = ref["occ"]
        assert np.isfinite(gx64).all() and np.isfinite(gy64).all()
        for w in ("a", "b"):
            gam, glm = ref["grads"][w]
            assert np.isfinite(gam).all() and np.isfinite(glm).all(), (what, w)
            if c["masked_lm"] is not None:      # -inf columns take no gradient, in either operand
                assert not gam[:, :, c["masked_am"]].any() and not glm[:, :, c["masked_lm"]].any()
            fam, flm = BC.float32_grads(c, builder, rnnt_type, ref["weights"][w])
            for b in range(B):          # the float32 floor: a tenth of the GPU tolerance
                e = max(BC.norm_err(fam[b], gam[b]), BC.norm_err(flm[b], glm[b]))
                assert e <= 1e-5, (what, w, b, e)
        gam, glm = ref["grads"]["b"]        # d loss / d am, d loss / d lm: zero outside the boundary, softmax gradients inside
        for b in range(B):
            se, te = int(c["boundary"][b, 2]), int(c["boundary"][b, 3])
            assert not gam[b, te:].any()
            if builder is None:     # (the smoothed builder's batch-wide unigram mean reaches every lm row)
                assert not glm[b, se + 1:].any()
            assert np.abs(gam[b].sum(axis=1)).max() <= 1e-9 * max(np.abs(gam[b]).max(), 1.0)
            assert np.abs(glm[b].sum(axis=1)).max() <= 1e-9 * max(np.abs(glm[b]).max(), 1.0)


@pytest.mark.parametrize("kind", BC.UNSOUND)
def test_unsound_kinds_have_no_float32_gradient(oracle, kind):
    """Why nothing is asserted about the GPU's gradients there: the reference arithmetic g / (prod + tiny) overflows and
    meets a zero (inf * 0), so the float32 restatement itself returns NaN."""
    shape = BC.SHAPES[0]
    c = BC.make_case(kind, shape, False)
    fam, flm = BC.float32_grads(c, None, "regular", BC.random_weights(c, "regular"))
    assert not (np.isfinite(fam).all() and np.isfinite(flm).all())
    # ... but the padding still takes none when the upstream gradient leaves it alone: 0 / (0 + tiny) is 0, where 0 / 0 is not
    for builder in (None, (0.1, 0.2)):
        fam, flm = BC.float32_grads(c, builder, "regular", BC.boundary_weights(c, "regular"))
        for b in range(c["B"]):
            se, te = int(c["boundary"][b, 2]), int(c["boundary"][b, 3])
            assert not fam[b, te:].any() and (builder is not None or not flm[b, se + 1:].any())


CHAIN_SHAPES = [(2, 130, 20, 37), (2, 72, 33, 36)]


@pytest.mark.parametrize("rnnt_type", BC.TYPES)
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=BC.shape_id)
def test_oracle_band_does_not_follow_the_planted_path(oracle, shape, rnnt_type):
    """Why the chain test of test_gpu_builder_structured.py does not ask that the planted path of agree12 lies inside the
    pruning band: the oracle's own ranges from the float64 occupancies do not contain it, for r = 3, 5 or 8.  With an
    additive joiner and a prediction network that is sure of the next symbol, a symbol step at a frame where am says blank
    costs what the blank step costs there (am[blank] + lm[sym] in both numerators, log(e^12 + e^12) below), so the
    posterior spreads over early emissions and the band follows the posterior.  (For the same reason agree12 is no
    low-loss model: its losses run from 18 to several hundred.)"""
    ref = BC.reference(oracle, "agree12", shape, rnnt_type, None)
    c = ref["case"]
    gx64, gy64 = ref["occ"]
    assert (-ref["ans64"]).min() > 10.0
    for r in (3, 5, 8):
        ranges = oracle.get_rnnt_prune_ranges(gx64.astype(np.float32), gy64.astype(np.float32), c["boundary"], r)
        nodes = BC.path_nodes(c, 0, rnnt_type)          # utterance 0, full size
        outside = sum(not ranges[0, t, 0] <= s <= ranges[0, t, r - 1] for s, t in nodes)
        assert outside > len(nodes) // 4, (r, outside, len(nodes))


def _pruned_lattice_loss_torch(x, sym, ranges, blank, bd, rnnt_type):
    """Sum over utterances of -log(total path probability) of pruned joiner logits x [B,T,r,C] (float64, autograd): px / py
    of rnnt_loss.py:853-1020 cell by cell (-inf outside the band: no such transition), px += py[1:] for the constrained type,
    and the log-domain lattice DP."""
    B, T, r, C = x.shape
    S = sym.shape[1]
    lp = x - torch.logsumexp(x, dim=3, keepdim=True)
    total = x.new_zeros(())
    for b in range(B):
        px, py = {}, {}
        for t in range(T):
            for k in range(r):
                s = int(ranges[b, t, k])
                py[(s, t)] = lp[b, t, k, blank]
                if s < S:
                    px[(s, t)] = lp[b, t, k, int(sym[b, s])]
        if rnnt_type == "constrained":
            px = {(s, t): v + py[(s + 1, t)] for (s, t), v in px.items() if (s + 1, t) in py}
        sb, tb, se, te = (int(v) for v in bd[b])
        p = {(sb, tb): x.new_zeros(())}
        for s in range(sb, se + 1):
            for t in range(tb, te + 1):
                terms = []
                tt = t if rnnt_type == "regular" else t - 1
                if s > sb and (s - 1, tt) in p and (s - 1, tt) in px and (rnnt_type != "regular" or tt < te):
                    terms.append(p[(s - 1, tt)] + px[(s - 1, tt)])
                if t > tb and (s, t - 1) in p and (s, t - 1) in py:
                    terms.append(p[(s, t - 1)] + py[(s, t - 1)])
                if terms:
                    p[(s, t)] = torch.logsumexp(torch.stack(terms), 0)
        total = total - p[(se, te)]
    return total


@pytest.mark.parametrize("rnnt_type", ["modified", "constrained"])
def test_pruned_gradient_of_the_oracle_on_a_band(oracle, rnnt_type):
    """oracle.rnnt_loss_pruned_grad on a real band (r = 3 < S + 1) against float64 autograd through the cell-by-cell
    restatement above: the constrained type (px = px' + py[1:]: what reaches px also reaches py one row below), and the
    modified type as the check of the restatement itself."""
    rng = np.random.default_rng(6)
    B, T, S, C, r = 2, 9, 5, 6, 3
    x = rng.standard_normal((B, T, r, C)).astype(np.float32)
    sym = rng.integers(0, C - 1, (B, S)).astype(np.int32)
    bd = np.array([[0, 0, S, T], [0, 0, S - 1, T - 2]], np.int32)
    s0 = np.minimum(np.arange(T) * (S + 1 - r) // (T - 3), S + 1 - r)
    ranges = (s0[None, :, None] + np.arange(r)[None, None, :]).astype(np.int32).repeat(B, axis=0)
    loss, g = oracle.rnnt_loss_pruned_grad(x, sym, ranges, C - 1, bd, rnnt_type, reduction="sum", dtype=np.float64)
    xd = torch.from_numpy(x).double().requires_grad_(True)
    want = _pruned_lattice_loss_torch(xd, sym, ranges, C - 1, bd, rnnt_type)
    want.backward()
    want = float(want.detach())
    assert np.isfinite(want) and abs(float(loss) - want) <= 1e-5 * abs(want)
    assert np.abs(xd.grad.numpy()).max() > 0.1 and BC.norm_err(g, xd.grad.numpy()) <= 1e-5


def test_constrained_pruned_gradient_of_the_oracle(oracle):
    """oracle.rnnt_loss_pruned_grad for the constrained type (px = px' + py[1:]: what reaches px also reaches py one row
    below) against float64 autograd through the joint restatement and the log-domain lattice DP, on identity ranges."""
    import hat_restatement as H
    import torch_restatements as R
    rng = np.random.default_rng(5)
    B, T, S, C = 2, 7, 4, 6
    x = rng.standard_normal((B, T, S + 1, C)).astype(np.float32)
    sym = rng.integers(0, C - 1, (B, S)).astype(np.int32)
    bd = np.array([[0, 0, S, T], [0, 0, S - 1, T - 2]], np.int32)
    ranges = np.broadcast_to(np.arange(S + 1, dtype=np.int32), (B, T, S + 1)).copy()
    loss, g = oracle.rnnt_loss_pruned_grad(x, sym, ranges, C - 1, bd, "constrained", reduction="sum", dtype=np.float64)
    xd = torch.from_numpy(x).double().requires_grad_(True)
    px, py = R.get_rnnt_logprobs_joint_torch(xd, torch.from_numpy(sym), C - 1, torch.from_numpy(bd), "constrained")
    want = H.lattice_loss_torch(px, py, bd, "constrained").sum()
    want.backward()
    want = float(want.detach())
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert BC.norm_err(g, xd.grad.numpy()) <= 1e-5
