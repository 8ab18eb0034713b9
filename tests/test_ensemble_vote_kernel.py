"""Soft-vote kernel (csrc/ensemble_kernels.hip ensemble_vote_kernel) and its
CPU oracle ops.cpu.ensemble_vote.

Exact cases: 1, 2 or 4 members with equal weights (1, 1/2, 1/4 after the
normalisation) and probabilities in eighths.  Every product and every
partial sum is then a multiple of 1/32 below 2, exact in f32 whether or not
the multiply-add is fused, so avg, label and conf must equal the oracle's
bit for bit, and exact ties pin the first-maximum rule.

Inexact cases: M members with random positive weights and Dirichlet rows
against an f64 average, atol = M * 2^-23.  The normalised weights sum to 1
within M * 2^-25 (each is rounded to f32 once) and the probabilities are
<= 1, so every partial sum is <= 1 + M * 2^-25 and each of the M fused steps
rounds once, by at most 2^-24 (half an ulp of a value < 2): M * 2^-24.  The f64
reference uses the same f32 weights, so the weight roundings cancel; what
is left of the bound, another M * 2^-24, covers the reference being formed
from the true quotients instead.  label and conf are functions of the
returned avg alone and are checked exactly against it.
"""

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROWS = (1, 255, 256, 257, 1500)  # 256 rows per block: partial, full, second block


def _og():
    from traffic_classifier_sdn_amd.ops import gpu as og

    return og


def _caps(monkeypatch):
    for cap in (None, 2):
        if cap is None:
            monkeypatch.delenv("TCSDN_PROBA_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("TCSDN_PROBA_BLOCKS", str(cap))
        yield cap


def _eighths(rng, n, C):
    """Rows of C multiples of 1/8 that sum to 1."""
    cuts = np.sort(rng.integers(0, 9, size=(n, C - 1)), axis=1)
    parts = np.diff(np.concatenate([np.zeros((n, 1), int), cuts, np.full((n, 1), 8)], axis=1), axis=1)
    return torch.from_numpy((parts / 8.0).astype(np.float32))


def _f64_vote(probas, colmaps, w32, C):
    avg = torch.zeros(probas[0].shape[0], C, dtype=torch.float64)
    for p, cmap, w in zip(probas, colmaps, w32):
        for j, col in enumerate(cmap):
            avg[:, col] += w * p[:, j].double()
    return avg


# ----------------------------------------------------------------------
# CPU oracle
# ----------------------------------------------------------------------


def test_oracle_missing_classes_and_order():
    # member 0 knows all three classes, member 1 only classes 2 and 0, in
    # that order
    p0 = torch.tensor([[0.5, 0.25, 0.25], [0.0, 1.0, 0.0]])
    p1 = torch.tensor([[0.75, 0.25], [0.5, 0.5]])
    avg, label, conf = oc.ensemble_vote([p0, p1], [[0, 1, 2], [2, 0]], None, 3)
    want = torch.tensor([[0.375, 0.125, 0.5], [0.25, 0.5, 0.25]])
    assert avg.dtype == torch.float32 and torch.equal(avg, want)
    assert label.dtype == torch.int32 and label.tolist() == [2, 1]
    assert conf.dtype == torch.float32 and conf.tolist() == [0.5, 0.5]
    none, label2, conf2 = oc.ensemble_vote([p0, p1], [[0, 1, 2], [2, 0]], None, 3, want_proba=False)
    assert none is None and torch.equal(label2, label) and torch.equal(conf2, conf)


def test_oracle_first_maximum_on_ties():
    p = torch.tensor([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.25, 0.5, 0.25]])
    _, label, conf = oc.ensemble_vote([p], [[0, 1, 2]], [3.0], 3)
    assert label.tolist() == [0, 1, 1] and conf.tolist() == [0.5, 0.5, 0.5]
    # the map moves the ties: row 0 ties on ensemble columns 2 and 0, row 1
    # on columns 0 and 1; the lower column wins, not the member's first
    _, label, _ = oc.ensemble_vote([p], [[2, 0, 1]], None, 3)
    assert label.tolist() == [0, 0, 0]
    _, label, _ = oc.ensemble_vote([p], [[1, 2, 0]], None, 3)
    assert label.tolist() == [1, 0, 2]


def test_weight_normalisation():
    assert oc.ensemble_weights(None, 4) == [0.25] * 4
    assert oc.ensemble_weights([2, 1, 1], 3) == [0.5, 0.25, 0.25]
    w = oc.ensemble_weights([1, 1, 1], 3)
    assert w == [float(np.float32(1.0 / 3.0))] * 3  # f64 quotient, rounded to f32 once
    w = oc.ensemble_weights([0.3, 1.7, 2.2, 0.9, 5.0], 5)
    assert abs(sum(w) - 1.0) <= 5 * 2.0 ** -25
    assert all(float(np.float32(v)) == v for v in w)
    p = torch.tensor([[0.5, 0.5], [1.0, 0.0]])
    a, _, _ = oc.ensemble_vote([p, p], [[0, 1], [0, 1]], [6.0, 2.0], 2)
    b, _, _ = oc.ensemble_vote([p, p], [[0, 1], [0, 1]], [0.75, 0.25], 2)
    assert torch.equal(a, b) and torch.equal(a, p)


P2 = torch.tensor([[0.5, 0.5]])
BAD = [
    ("no members", dict(probas=[], colmaps=[], weights=None, C=2)),
    ("nine members", dict(probas=[P2] * 9, colmaps=[[0, 1]] * 9, weights=None, C=2)),
    ("one class", dict(probas=[P2], colmaps=[[0, 0]], weights=None, C=1)),
    ("nine classes", dict(probas=[P2], colmaps=[[0, 1]], weights=None, C=9)),
    ("map entry == C", dict(probas=[P2], colmaps=[[0, 2]], weights=None, C=2)),
    ("negative map entry", dict(probas=[P2], colmaps=[[0, -1]], weights=None, C=2)),
    ("short map", dict(probas=[P2], colmaps=[[0]], weights=None, C=2)),
    ("missing map", dict(probas=[P2, P2], colmaps=[[0, 1]], weights=None, C=2)),
    ("different n", dict(probas=[P2, P2.repeat(2, 1)], colmaps=[[0, 1]] * 2, weights=None, C=2)),
    ("nine member classes", dict(probas=[torch.full((1, 9), 1 / 9)], colmaps=[[0] * 9], weights=None, C=2)),
    ("nan weight", dict(probas=[P2, P2], colmaps=[[0, 1]] * 2, weights=[1.0, float("nan")], C=2)),
    ("inf weight", dict(probas=[P2, P2], colmaps=[[0, 1]] * 2, weights=[1.0, float("inf")], C=2)),
    ("zero weight", dict(probas=[P2, P2], colmaps=[[0, 1]] * 2, weights=[1.0, 0.0], C=2)),
    ("negative weight", dict(probas=[P2, P2], colmaps=[[0, 1]] * 2, weights=[2.0, -1.0], C=2)),
    ("zero total", dict(probas=[P2], colmaps=[[0, 1]], weights=[0.0], C=2)),
    ("weight count", dict(probas=[P2, P2], colmaps=[[0, 1]] * 2, weights=[1.0], C=2)),
]


@pytest.mark.parametrize("case", BAD, ids=[b[0] for b in BAD])
def test_oracle_errors(case):
    kw = case[1]
    with pytest.raises(ValueError):
        oc.ensemble_vote(kw["probas"], kw["colmaps"], kw["weights"], kw["C"])


@needs_gpu
@pytest.mark.gpu
def test_gpu_errors():
    """The binding applies the oracle's rules, and the extension entry point
    has its own checks behind them."""
    og = _og()
    for _, kw in BAD:
        with pytest.raises(ValueError):
            og.ensemble_vote([p.cuda() for p in kw["probas"]], kw["colmaps"], kw["weights"], kw["C"])
    p = P2.cuda()
    ext = og._ext.ensemble_vote
    for args in (
        ([p] * 9, [[0, 1]] * 9, [1 / 9] * 9, 2),
        ([p], [[0, 1]], [1.0], 9),
        ([p], [[0, 2]], [1.0], 2),
        ([p, p.repeat(2, 1)], [[0, 1]] * 2, [0.5, 0.5], 2),
        ([p], [[0, 1]], [float("nan")], 2),
        ([p], [[0, 1]], [0.0], 2),
    ):
        with pytest.raises(RuntimeError):
            ext(*args, True)


# ----------------------------------------------------------------------
# GPU, exact
# ----------------------------------------------------------------------


def _exact_case(M, C, seed):
    """M members in eighths with permuted maps into C ensemble columns: the
    first covers all C, the second C - 1 (where that is still two), the
    others 2..C.  Rows 0..3 tie exactly: the first member puts half on each
    of two columns and the others nothing (the kernel does not ask for rows
    that sum to one)."""
    rng = np.random.default_rng(seed)
    n = max(ROWS)
    sizes = [C] + [max(2, C - 1)] * (M > 1) + [int(rng.integers(2, C + 1)) for _ in range(M - 2)]
    probas, colmaps = [], []
    for cm in sizes:
        probas.append(_eighths(rng, n, cm))
        colmaps.append([int(c) for c in rng.permutation(C)[:cm]])
    for i, p in enumerate(probas):
        p[:4] = 0.0
        if i == 0:
            for r in range(4):
                a, b = rng.choice(C, size=2, replace=False)
                p[r, a] = p[r, b] = 0.5
    return probas, colmaps


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 6, 8])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_exact_vote(monkeypatch, M, C):
    og = _og()
    probas, colmaps = _exact_case(M, C, 100 * M + C)
    assert M == 1 or C == 2 or any(p.shape[1] < C for p in probas)
    ref_a, ref_l, ref_c = oc.ensemble_vote(probas, colmaps, None, C)
    # the oracle's ties are real: the best value is reached twice
    assert bool(((ref_a[:4] == ref_c[:4].unsqueeze(1)).sum(dim=1) >= 2).all())
    dev = [p.cuda() for p in probas]
    for cap in _caps(monkeypatch):
        for n in ROWS:
            tag = f"M {M} C {C} cap {cap} n {n}"
            avg, label, conf = og.ensemble_vote([p[:n] for p in dev], colmaps, None, C)
            assert avg.dtype == torch.float32 and avg.shape == (n, C), tag
            assert label.dtype == torch.int32 and conf.dtype == torch.float32, tag
            assert torch.equal(avg.cpu(), ref_a[:n]), tag
            assert torch.equal(label.cpu(), ref_l[:n]), tag
            assert torch.equal(conf.cpu(), ref_c[:n]), tag


# ----------------------------------------------------------------------
# GPU, inexact
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("M", [3, 5, 8])
def test_inexact_vote(monkeypatch, M):
    og = _og()
    rng = np.random.default_rng(200 + M)
    C, n = 6, max(ROWS)
    sizes = [6, 4, 5, 2, 6, 3, 6, 4][:M]
    probas = [torch.from_numpy(rng.dirichlet(np.ones(cm), size=n).astype(np.float32)) for cm in sizes]
    colmaps = [[int(c) for c in rng.permutation(C)[:cm]] for cm in sizes]
    weights = [float(w) for w in rng.uniform(0.2, 5.0, size=M)]
    w32 = oc.ensemble_weights(weights, M)
    ref = _f64_vote(probas, colmaps, w32, C)
    atol = M * 2.0 ** -23
    oracle_err = float((oc.ensemble_vote(probas, colmaps, weights, C)[0].double() - ref).abs().max())
    assert oracle_err <= atol
    dev = [p.cuda() for p in probas]
    for cap in _caps(monkeypatch):
        for rows in ROWS:
            tag = f"M {M} cap {cap} n {rows}"
            avg, label, conf = og.ensemble_vote([p[:rows] for p in dev], colmaps, weights, C)
            err = float((avg.cpu().double() - ref[:rows]).abs().max())
            print(f"{tag}: max err {err:.3e} (atol {atol:.3e})")
            assert err <= atol, tag
            avg_h = avg.cpu()
            best = avg_h.max(dim=1).values
            first = torch.argmax((avg_h == best.unsqueeze(1)).to(torch.uint8), dim=1).to(torch.int32)
            assert torch.equal(conf.cpu(), best), tag
            assert torch.equal(label.cpu(), first), tag
            none, label2, conf2 = og.ensemble_vote(
                [p[:rows] for p in dev], colmaps, weights, C, want_proba=False)
            assert none is None, tag
            assert torch.equal(label2, label) and torch.equal(conf2, conf), tag


@needs_gpu
@pytest.mark.gpu
def test_vote_captures():
    """No sync and no allocation beyond the outputs: the launch captures,
    and a replay over new member probabilities gives the eager result."""
    og = _og()
    rng = np.random.default_rng(300)
    n, C = 2048, 6
    sizes = (6, 6, 4)
    colmaps = [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [0, 2, 4, 5]]
    make = lambda: [torch.from_numpy(rng.dirichlet(np.ones(cm), size=n).astype(np.float32)).cuda()
                    for cm in sizes]
    static, other = make(), make()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            og.ensemble_vote(static, colmaps, [2, 1, 1], C)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = og.ensemble_vote(static, colmaps, [2, 1, 1], C)
    for a, b in zip(static, other):
        a.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, og.ensemble_vote(other, colmaps, [2, 1, 1], C)):
        assert torch.equal(got, want)
