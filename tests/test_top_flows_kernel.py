"""Top talkers per class (csrc/top_flows_kernels.hip) and the CPU oracle
ops.cpu.class_top_flows.

A key is a sum of f32 adds in a stated order and the order of the flows is a
total one (larger key, then lower row), so the oracle and the kernel give the
same bits: every comparison here is equality, of the rows and of the keys.
Only where a NaN key is planted are the keys compared as "NaN in the same
cells, equal elsewhere", since a NaN equals nothing.
"""

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import ops
from traffic_classifier_sdn_amd.ops import cpu as oc

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# a wave takes 64 rows and a block 256: partial, full and second tiles of both
ROWS = (1, 63, 64, 65, 255, 256, 257, 1500)
CLASSES = (2, 6, 8)
KS = (1, 5, 64)  # 64: a full list of one cell per lane; with few rows it never fills
NAN, INF = float("nan"), float("inf")


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


def _live(v, device="cpu"):
    return torch.tensor([v], dtype=torch.int32, device=device)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _keyed(keys, col=4):
    """[n, 12] f32, zero but for ``keys`` in column ``col``."""
    X = torch.zeros(len(keys), 12)
    X[:, col] = torch.tensor(keys, dtype=torch.float32)
    return X


def _same(got, want):
    """Rows equal; keys equal, a NaN matching a NaN."""
    (gr, gk), (wr, wk) = got, want
    gr, gk, wr, wk = gr.cpu(), gk.cpu(), wr.cpu(), wk.cpu()
    if not (gr.dtype == wr.dtype == torch.int32 and gk.dtype == wk.dtype == torch.float32):
        return False
    gn, wn = torch.isnan(gk), torch.isnan(wk)
    zero = torch.zeros_like(gk)
    return (torch.equal(gr, wr) and torch.equal(gn, wn)
            and torch.equal(torch.where(gn, zero, gk), torch.where(wn, zero, wk)))


# ----------------------------------------------------------------------
# CPU oracle: one hand-written case per rule
# ----------------------------------------------------------------------


def test_default_columns_are_the_byte_rates():
    assert oc.TOP_FLOW_COLUMNS == (4, 10)
    assert ops.TOP_FLOW_COLUMNS is oc.TOP_FLOW_COLUMNS
    assert oc.TRAFFIC_COLUMNS[1 + 4] == "Forward Instantaneous Bytes per Second"
    assert oc.TRAFFIC_COLUMNS[1 + 10] == "Reverse Instantaneous Bytes per Second"


def test_oracle_five_rows_in_two_classes():
    X = _keyed([10.0, 50.0, 30.0, 20.0, 40.0])
    rows, keys = oc.class_top_flows(X, _i32([0, 1, 0, 1, 1]), 2, 2)
    assert rows.dtype == torch.int32 and keys.dtype == torch.float32
    assert rows.tolist() == [[2, 0], [1, 4], [-1, -1]]
    assert keys.tolist() == [[30.0, 10.0], [50.0, 40.0], [0.0, 0.0]]
    rows, keys = ops.class_top_flows(X, _i32([0, 1, 0, 1, 1]), 2, 3)
    assert rows.tolist() == [[2, 0, -1], [1, 4, 3], [-1, -1, -1]]
    assert keys.tolist() == [[30.0, 10.0, 0.0], [50.0, 40.0, 20.0], [0.0, 0.0, 0.0]]


def test_oracle_equal_keys_go_by_the_lower_row():
    X = _keyed([7.0, 9.0, 7.0, 9.0, 7.0, 9.0])
    rows, keys = oc.class_top_flows(X, _i32([0] * 6), 2, 4)
    assert rows[0].tolist() == [1, 3, 5, 0]
    assert keys[0].tolist() == [9.0, 9.0, 9.0, 7.0]


def test_oracle_fewer_than_k_rows_are_padded():
    rows, keys = oc.class_top_flows(_keyed([3.0, 4.0]), _i32([1, 1]), 3, 5)
    assert rows.tolist() == [[-1] * 5, [1, 0, -1, -1, -1], [-1] * 5, [-1] * 5]
    assert keys[1].tolist() == [4.0, 3.0, 0.0, 0.0, 0.0] and not bool(keys[[0, 2, 3]].any())


def test_oracle_out_of_range_labels_are_unknown():
    X = _keyed([1.0, 2.0, 3.0, 4.0, 5.0])
    rows, keys = oc.class_top_flows(X, _i32([-1, -(2**31), 3, 2**31 - 1, 1]), 3, 5)
    assert rows.tolist() == [[-1] * 5, [4, -1, -1, -1, -1], [-1] * 5, [3, 2, 1, 0, -1]]
    assert keys[3].tolist() == [4.0, 3.0, 2.0, 1.0, 0.0]


def test_oracle_low_confidence_is_unknown_and_nan_is_not():
    X = _keyed([1.0, 2.0, 4.0, 8.0])
    conf = torch.tensor([0.5, 0.25, NAN, 0.75])
    rows, _ = oc.class_top_flows(X, _i32([0, 0, 0, 1]), 2, 3, conf=conf, min_conf=0.5)
    # 0.5 < 0.5 is false, 0.25 < 0.5 true, NaN < 0.5 false
    assert rows.tolist() == [[2, 0, -1], [3, -1, -1], [1, -1, -1]]
    # the comparison is made with f32(min_conf): 0.1f is above 0.1
    conf = torch.full((4,), 0.1)
    rows, _ = oc.class_top_flows(X, _i32([0, 0, 0, 1]), 2, 3, conf=conf, min_conf=0.1)
    assert rows[2].tolist() == [-1, -1, -1]


@pytest.mark.parametrize("live, listed", [(0, []), (1, [0]), (4, [3, 2, 1, 0]), (9, [3, 2, 1, 0])])
def test_oracle_n_live(live, listed):
    X = _keyed([1.0, 2.0, 4.0, 8.0])
    X[live:] = NAN  # a dead row is no candidate, and a NaN would rank first
    rows, keys = oc.class_top_flows(X, _i32([0, 0, 0, 0]), 2, 4, n_live=_live(live))
    assert rows[0].tolist() == listed + [-1] * (4 - len(listed))
    assert bool(torch.isfinite(keys).all()) and not bool((rows[1:] != -1).any())


def test_oracle_nan_first_and_minus_inf_last():
    X = _keyed([1.0, INF, -INF, NAN, -5.0, -NAN, 0.0])
    rows, keys = oc.class_top_flows(X, _i32([0] * 7), 2, 7)
    assert rows[0].tolist() == [3, 5, 1, 0, 6, 4, 2]  # the NaNs tie: lower row first
    assert torch.isnan(keys[0, :2]).all()
    assert keys[0, 2:].tolist() == [INF, 1.0, 0.0, -5.0, -INF]


def test_oracle_plus_and_minus_zero_tie():
    rows, _ = oc.class_top_flows(_keyed([-0.0, 0.0, -0.0, 0.0, -1.0]), _i32([1] * 5), 2, 5)
    assert rows[1].tolist() == [0, 1, 2, 3, 4]


def test_oracle_key_is_the_f32_sum_in_column_order():
    rng = np.random.default_rng(5)
    X = torch.from_numpy(np.exp(rng.normal(8.0, 4.0, size=(40, 12))).astype(np.float32))
    lab = torch.zeros(40, dtype=torch.int32)
    rows, keys = oc.class_top_flows(X, lab, 2, 40)
    want = X[:, 4] + X[:, 10]
    assert want.dtype == torch.float32
    assert torch.equal(keys[0], want[rows[0].long()])
    assert torch.equal(keys[0], want.sort(descending=True).values)
    # three columns where the order of the f32 adds decides the sum
    X = torch.zeros(2, 12)
    X[0, :3] = torch.tensor([1e8, 1.0, -1e8])  # (1e8 + 1) - 1e8 = 0 in f32
    X[1, :3] = torch.tensor([1e8, -1e8, 1.0])  # (1e8 - 1e8) + 1 = 1
    for columns in ((0, 1, 2), (2, 0, 1)):  # ascending column order, however they are named
        rows, keys = oc.class_top_flows(X, _i32([0, 0]), 2, 2, columns=columns)
        assert rows[0].tolist() == [1, 0] and keys[0].tolist() == [1.0, 0.0]


def test_oracle_no_rows():
    rows, keys = oc.class_top_flows(torch.zeros(0, 12), _i32([]), 6, 3)
    assert tuple(rows.shape) == tuple(keys.shape) == (7, 3)
    assert bool((rows == -1).all()) and not bool(keys.any())


def _bad_cases(device):
    X = torch.zeros(4, 12, device=device)
    lab = torch.zeros(4, dtype=torch.int32, device=device)
    conf = torch.zeros(4, device=device)
    cols = (4, 10)
    other = "cpu" if device != "cpu" else "meta"
    return [
        ("k of 0", lambda: (X, lab, 3, 0)),
        ("k of 65", lambda: (X, lab, 3, 65)),
        ("float k", lambda: (X, lab, 3, 2.0)),
        ("one class", lambda: (X, lab, 1, 2)),
        ("nine classes", lambda: (X, lab, 9, 2)),
        ("no columns", lambda: (X, lab, 3, 2, ())),
        ("a column twice", lambda: (X, lab, 3, 2, (4, 4))),
        ("column 12", lambda: (X, lab, 3, 2, (4, 12))),
        ("column -1", lambda: (X, lab, 3, 2, (-1,))),
        ("float column", lambda: (X, lab, 3, 2, (4.0,))),
        ("columns as an int", lambda: (X, lab, 3, 2, 4)),
        ("11 features", lambda: (X[:, :11].contiguous(), lab, 3, 2)),
        ("f64 X", lambda: (X.double(), lab, 3, 2)),
        ("int64 labels", lambda: (X, lab.long(), 3, 2)),
        ("short labels", lambda: (X, lab[:3], 3, 2)),
        ("strided X", lambda: (torch.zeros(4, 24, device=device)[:, ::2], lab, 3, 2)),
        ("strided labels", lambda: (X, torch.zeros(8, dtype=torch.int32, device=device)[::2], 3, 2)),
        ("labels elsewhere", lambda: (X, lab.to(other), 3, 2)),
        ("f64 conf", lambda: (X, lab, 3, 2, cols, conf.double(), 0.5)),
        ("short conf", lambda: (X, lab, 3, 2, cols, conf[:3], 0.5)),
        ("strided conf", lambda: (X, lab, 3, 2, cols, torch.zeros(8, device=device)[::2], 0.5)),
        ("conf elsewhere", lambda: (X, lab, 3, 2, cols, conf.to(other), 0.5)),
        ("nan min_conf", lambda: (X, lab, 3, 2, cols, conf, NAN)),
        ("min_conf past f32", lambda: (X, lab, 3, 2, cols, conf, 1e39)),
        ("int n_live", lambda: (X, lab, 3, 2, cols, None, 0.0, 2)),
        ("int64 n_live", lambda: (X, lab, 3, 2, cols, None, 0.0, torch.tensor([2], device=device))),
        ("scalar n_live", lambda: (X, lab, 3, 2, cols, None, 0.0,
                                   torch.tensor(2, dtype=torch.int32, device=device))),
        ("n_live elsewhere", lambda: (X, lab, 3, 2, cols, None, 0.0, _live(2, other))),
    ]


@pytest.mark.parametrize("case", _bad_cases("cpu"), ids=lambda c: c[0])
def test_oracle_refusals(case):
    with pytest.raises(ValueError):
        oc.class_top_flows(*case[1]())


# ----------------------------------------------------------------------
# GPU against the oracle
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_gpu_refusals():
    og = _og()
    for name, make in _bad_cases("cuda"):
        with pytest.raises(ValueError):
            og.class_top_flows(*make())
    # the extension entry point has its own checks behind the shared ones
    X = torch.zeros(4, 12, device="cuda")
    lab = torch.zeros(4, dtype=torch.int32, device="cuda")
    ext = og._ext.selection.class_top_flows
    mask = (1 << 4) | (1 << 10)
    for C, k in ((9, 2), (1, 2), (3, 0), (3, 65)):
        with pytest.raises(RuntimeError, match="no kernel for"):
            ext(X, lab, C, k, mask, None, 0.0, None)
    for args in (
        (X.double(), lab, 3, 2, mask, None, 0.0, None),
        (X, lab[:3], 3, 2, mask, None, 0.0, None),
        (X, lab.long(), 3, 2, mask, None, 0.0, None),
        (X, lab, 3, 2, mask, torch.zeros(3, device="cuda"), 0.0, None),
        (X, lab, 3, 2, mask, torch.zeros(4, device="cuda").double(), 0.0, None),
        (X, lab, 3, 2, 0, None, 0.0, None),
        (X, lab, 3, 2, 1 << 12, None, 0.0, None),
        (X, lab, 3, 2, mask, None, NAN, None),
        (X, lab, 3, 2, mask, None, 0.0, torch.tensor([2], device="cuda")),
        (X.cpu(), lab, 3, 2, mask, None, 0.0, None),
    ):
        with pytest.raises(RuntimeError):
            ext(*args)


def _labels(rng, n, C):
    """Mostly classes, with out-of-range values of every kind mixed in."""
    lab = rng.integers(0, C, size=n).astype(np.int64)
    odd = rng.random(n) < 0.15
    lab[odd] = rng.choice([-1, -(2**31), C, C + 1, 2**31 - 1], size=int(odd.sum()))
    return torch.from_numpy(lab.astype(np.int32))


def _conf(rng, n):
    conf = rng.random(n).astype(np.float32)
    conf[rng.random(n) < 0.05] = np.nan
    conf[rng.random(n) < 0.05] = 0.5  # equal to min_conf: not below it
    return torch.from_numpy(conf)


def _lognormal(rng, n):
    return torch.from_numpy(np.exp(rng.normal(8.0, 4.0, size=(n, 12))).astype(np.float32))


def _with_keys(rng, n, fwd, rev):
    """Random features, so that a wrong column shows, with the two key columns set."""
    X = _lognormal(rng, n)
    X[:, 4] = torch.as_tensor(fwd, dtype=torch.float32)
    X[:, 10] = torch.as_tensor(rev, dtype=torch.float32)
    return X


def _data(name, rng, n, C):
    """(X, labels) of one data set of the sweep."""
    lab = _labels(rng, n, C)
    if name == "ties":  # integer keys 0..7: nearly every comparison is a tie
        return _with_keys(rng, n, rng.integers(0, 4, n), rng.integers(0, 5, n)), lab
    if name == "lognormal":
        return _lognormal(rng, n), lab
    if name == "equal":  # all keys equal: the row rule alone
        return _with_keys(rng, n, np.full(n, 3.0), np.full(n, 5.0)), lab
    # one class, keys strictly ascending (or descending) in row order: on the
    # way up every row of a tile beats the list and is inserted
    r = np.arange(n, dtype=np.float32)
    r = r if name == "ascending" else r[::-1].copy()
    return _with_keys(rng, n, r, r), torch.zeros(n, dtype=torch.int32)


DATA = ("ties", "lognormal", "ascending", "descending", "equal")


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", DATA)
def test_gpu_equals_oracle(monkeypatch, name, C):
    og = _og()
    rng = np.random.default_rng(1700 + 10 * DATA.index(name) + C)
    n_max = max(ROWS)
    X, lab = _data(name, rng, n_max, C)
    conf = _conf(rng, n_max)
    dX, dlab, dconf = X.cuda(), lab.cuda(), conf.cuda()
    want = {}
    for cap in _caps(monkeypatch):
        for n in ROWS:
            for k in KS:
                for use_conf in (False, True):
                    for live in (None, 0, 1, n - 1, n):
                        key = (n, k, use_conf, live)
                        if key not in want:  # the oracle does not depend on the cap
                            want[key] = oc.class_top_flows(
                                X[:n], lab[:n], C, k, conf=conf[:n] if use_conf else None,
                                min_conf=0.5, n_live=None if live is None else _live(live))
                        rows, keys = og.class_top_flows(
                            dX[:n], dlab[:n], C, k, conf=dconf[:n] if use_conf else None,
                            min_conf=0.5, n_live=None if live is None else _live(live, "cuda"))
                        tag = f"{name} C {C} cap {cap} n {n} k {k} conf {use_conf} live {live}"
                        assert rows.dtype == torch.int32 and tuple(rows.shape) == (C + 1, k), tag
                        assert keys.dtype == torch.float32 and tuple(keys.shape) == (C + 1, k), tag
                        assert torch.equal(rows.cpu(), want[key][0]), tag
                        assert torch.equal(keys.cpu(), want[key][1]), tag
                        m = n if live is None else live
                        assert int((rows >= 0).sum()) <= m, tag
    full = want[(n_max, 64, False, None)][0]
    if name in ("ascending", "descending"):  # class 0 alone, its list full
        top = list(range(n_max - 1, n_max - 65, -1)) if name == "ascending" else list(range(64))
        assert full[0].tolist() == top and bool((full[1:] == -1).all())


@needs_gpu
@pytest.mark.gpu
def test_gpu_planted_nan_and_infinities(monkeypatch):
    og = _og()
    rng = np.random.default_rng(1800)
    n, C, k = 700, 6, 5
    X, lab = _lognormal(rng, n), _labels(rng, n, C)
    lab[[70, 333, 334, 600, 650, 651]] = 2
    X[333, 4] = NAN
    X[600, 10] = -NAN  # the sign bit of a NaN does not matter
    X[70, 4] = INF
    X[650, 4], X[650, 10] = INF, -INF  # inf - inf: a NaN made by the adds
    X[[334, 651], 4] = -INF
    want = oc.class_top_flows(X, lab, C, k)
    assert want[0][2].tolist()[:4] == [333, 600, 650, 70]
    assert not bool(((want[0] == 334) | (want[0] == 651)).any())
    kall = 64  # a class 2 of five rows, so that its last ones are listed too
    lab2 = torch.full_like(lab, 1)
    lab2[[10, 20, 30, 334, 651]] = 2
    last = oc.class_top_flows(X, lab2, C, kall)
    assert last[0][2].tolist()[3:5] == [334, 651]  # -inf last, the lower row first
    for cap in _caps(monkeypatch):
        assert _same(og.class_top_flows(X.cuda(), lab.cuda(), C, k), want), cap
        assert _same(og.class_top_flows(X.cuda(), lab2.cuda(), C, kall), last), cap


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("columns", [(7,), (0, 5, 11), (3, 2, 1, 0), tuple(range(12))])
def test_gpu_other_columns(monkeypatch, columns):
    """Keys from one, two and all three quarters of a row, in the stated add
    order (the exp(N(8, 4)) values make a different order give other bits)."""
    og = _og()
    rng = np.random.default_rng(1900 + len(columns))
    n, C = 1500, 6
    X, lab = _lognormal(rng, n), _labels(rng, n, C)
    X[::3] *= -1.0
    for k in (5, 64):
        want = oc.class_top_flows(X, lab, C, k, columns=columns)
        for cap in _caps(monkeypatch):
            rows, keys = og.class_top_flows(X.cuda(), lab.cuda(), C, k, columns=columns)
            assert torch.equal(rows.cpu(), want[0]) and torch.equal(keys.cpu(), want[1]), (k, cap)


@needs_gpu
@pytest.mark.gpu
def test_gpu_no_rows_writes_padding():
    og = _og()
    rows, keys = og.class_top_flows(
        torch.zeros(0, 12, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 6, 64)
    assert tuple(rows.shape) == tuple(keys.shape) == (7, 64)
    assert bool((rows == -1).all()) and not bool(keys.any())


@needs_gpu
@pytest.mark.gpu
def test_result_does_not_depend_on_the_grid(monkeypatch):
    """Two calls agree, under both caps, and so do the capped and the
    uncapped grid."""
    og = _og()
    rng = np.random.default_rng(2000)
    n, C = 1500, 6
    X, lab, conf = _lognormal(rng, n).cuda(), _labels(rng, n, C).cuda(), _conf(rng, n).cuda()
    seen = []
    for cap in _caps(monkeypatch):
        a = og.class_top_flows(X, lab, C, 10, conf=conf, min_conf=0.5)
        b = og.class_top_flows(X, lab, C, 10, conf=conf, min_conf=0.5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), cap
        seen.append(a)
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])


@needs_gpu
@pytest.mark.gpu
def test_top_flows_capture():
    """One capture, replayed after X, labels, conf and n_live were overwritten
    in place, follows the new contents; a live count of 0 leaves padding, not
    the entries of the replay before."""
    og = _og()
    rng = np.random.default_rng(2100)
    n, C, k = 1500, 6, 10
    polls = [
        (_lognormal(rng, n).cuda(), _labels(rng, n, C).cuda(), _conf(rng, n).cuda(), live)
        for live in (n, 5, 0, 1000)
    ]
    sX, slab, sconf = (t.clone() for t in polls[0][:3])
    d_live = _live(n, "cuda")
    run = lambda: og.class_top_flows(sX, slab, C, k, conf=sconf, min_conf=0.5, n_live=d_live)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rows, keys = run()
    for i, (X, lab, conf, live) in enumerate(polls):
        sX.copy_(X)
        slab.copy_(lab)
        sconf.copy_(conf)
        d_live.fill_(live)
        g.replay()
        torch.cuda.synchronize()
        want = og.class_top_flows(X, lab, C, k, conf=conf, min_conf=0.5, n_live=_live(live, "cuda"))
        assert torch.equal(rows, want[0]) and torch.equal(keys, want[1]), i
        assert int(rows.max()) < max(live, 0) or live == 0, i
        cpu = oc.class_top_flows(X.cpu(), lab.cpu(), C, k, conf=conf.cpu(), min_conf=0.5,
                                 n_live=_live(live))
        assert torch.equal(rows.cpu(), cpu[0]) and torch.equal(keys.cpu(), cpu[1]), i
        if live == 0:
            assert bool((rows == -1).all()) and not bool(keys.any())
