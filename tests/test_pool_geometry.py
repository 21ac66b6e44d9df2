"""The pool library (vboc_amd/csrc/pool.hip) at the launch geometry of the AL loop and at the edge values its header
names: several rounds per workgroup of k_fwd, the grid-stride of k_hist, scan segments of k_scan longer than one block,
the special keys of the selection, the entropy's NaN / 0 log 0 / -0 rules, and scratch buffers that regrow on a live
handle.  The float64 restatements and bounds are tests/test_pool_device.py's.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_pool_device import (ETP_TOL, U, _scores, entropy64_of_logits, forward64, norm32, padded, params64, pool_rows,
                              scored, trained)

# the launch constants of vboc_amd/csrc/pool.hip (RT rows per workgroup and round of k_fwd, FWG its most workgroups,
# HG the most workgroups of k_hist (256 rows each), SB rows per workgroup of k_count / k_scatter); every n below
# follows from them
RT, FWG, HG, SB = 64, 2048, 1024, 2048
SCAN = 256                                  # threads of k_scan's one workgroup
N_FWD = 2 * RT * FWG + RT + 1               # 4098 tiles: workgroups 0 and 1 do three rounds, the last tile has one row
N_SEG2 = SB * 261 + 5                       # nblk 262, seg 2 (131 owning threads), k_hist does three grid rounds
N_SEG3 = SB * 514 + 5                       # nblk 515, seg 3 (the last owning thread's segment is short: 2 blocks)
CHUNK = RT * 1024                           # 1024 tiles: one round per workgroup


def test_the_sizes_reach_the_paths_they_are_named_for():
    tiles = -(-N_FWD // RT)
    assert N_FWD == 262209 and tiles == 4098 == 2 * FWG + 2 and N_FWD - (tiles - 1) * RT == 1
    assert CHUNK // RT <= FWG
    for n, seg, last in ((N_SEG2, 2, 2), (N_SEG3, 3, 2)):
        nblk = -(-n // SB)
        assert -(-nblk // SCAN) == seg and nblk - (nblk - 1) // seg * seg == last    # at N_SEG3 a short last segment
        assert nblk < SCAN * seg - seg                               # and threads that own no block at all
        assert n > 2 * HG * 256                                      # more than two grid rounds of k_hist
    assert (N_SEG2, N_SEG3) == (534533, 1052677)
    assert -(-(-(-70001 // SB)) // SCAN) == 1                        # what the older suite reaches


def sample_rows(n):
    return np.unique(np.r_[np.arange(0, n, 61), np.arange(max(n - 130, 0), n)])


# -- 1. the entropy over several rounds per workgroup -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nin,hidden", [(6, 500), (4, 300), (6, 33)])
def test_pool_entropy_over_several_rounds_per_workgroup(nin, hidden):
    model, mean, std = trained(nin, hidden)
    sc, X, Xd, etp, lg = scored(nin, hidden, N_FWD)
    assert etp.shape == (N_FWD,) and lg.shape == (N_FWD, 2)
    # every row against the one-round regime that test_pool_entropy_matches_float64_forward pins to float64
    parts = [sc.entropy(Xd[c:c + CHUNK].contiguous(), mean, std, logits=True) for c in range(0, N_FWD, CHUNK)]
    assert len(parts) == 5
    assert torch.equal(etp, torch.cat([p[0] for p in parts])) and torch.equal(lg, torch.cat([p[1] for p in parts]))
    rows = sample_rows(N_FWD)
    assert 4300 < len(rows) < 4500 and rows[-1] == N_FWD - 1
    H = padded(hidden)
    lg64, a3 = forward64(params64(model), norm32(X[rows], mean, std))
    tau = (nin + 2 * H + 3) * U * a3
    lgh = lg.cpu().numpy()[rows]
    err = np.abs(lgh.astype(np.float64) - lg64)
    print("logit error / bound", float((err / tau).max()))
    assert np.all(err <= tau)
    e = etp.cpu().numpy()[rows]
    assert np.all(np.isfinite(e)) and np.all(e >= 0) and not np.any(np.signbit(e))
    d = np.abs(e.astype(np.float64) - entropy64_of_logits(lgh))
    print("entropy error", float(d.max()), "spread", float(e.min()), float(e.max()))
    assert d.max() <= ETP_TOL


# -- 2. the labels ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nin,hidden,n", [(6, 33, 257), (6, 33, N_FWD), (6, 500, N_FWD)])
def test_pool_labels_are_the_logits_comparison(nin, hidden, n):
    """labels = l1 > l0 of the call's own logits, exactly; against float64 wherever the float64 logits are further
    apart than the two forward bounds together (there no float32 summation order can turn the comparison).  The rows
    nearer than that are left out: their count is printed and capped at 5 % of the sample.  The classifier of hidden
    33 never reaches l1 > l0 on this pool (its largest entropy is 0.687 < ln 2), so its labels are all 0; the one of
    hidden 500 has both."""
    from vboc_amd import poollib
    model, mean, std = trained(nin, hidden)
    sc, X, Xd, etp0, lg0 = scored(nin, hidden, n)
    lib = poollib.load()
    s = torch.cuda.current_stream().cuda_stream
    etp = torch.empty(n, dtype=torch.float32, device="cuda")
    lg = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    lab = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    poollib.check(lib.vboc_pool_set_classifier(sc._h, *sc._ptrs(model), s))
    poollib.check(lib.vboc_pool_entropy(sc._h, Xd.data_ptr(), n, mean, std, etp.data_ptr(), lg.data_ptr(),
                                        lab.data_ptr(), s))
    torch.cuda.synchronize()
    assert torch.equal(etp, etp0) and torch.equal(lg, lg0)
    assert torch.equal(lab, (lg[:, 1] > lg[:, 0]).to(torch.uint8))
    rows = sample_rows(n)
    lg64, a3 = forward64(params64(model), norm32(X[rows], mean, std))
    tau = (nin + 2 * padded(hidden) + 3) * U * a3
    clear = np.abs(lg64[:, 1] - lg64[:, 0]) > tau[:, 0] + tau[:, 1]
    out = int((~clear).sum())
    print("rows left out", out, "of", len(rows), "share", out / len(rows))
    assert out < 0.05 * len(rows)
    labh = lab.cpu().numpy()[rows]
    assert np.array_equal(labh[clear], (lg64[:, 1] > lg64[:, 0])[clear].astype(np.uint8))
    ones = int(lab.sum())
    print("rows labelled 1", ones, "of", n)
    if hidden == 500:
        assert 0 < ones < n and 0 < labh.sum() < len(rows)      # both labels occur, in the sample too


# -- 3. the entropy's edge values on a constructed classifier ---------------------------------------
EDGE_V = (-200, -120, -89, -88, -87, -80, -40, -17, -1, 0, 1, 17, 40, 88, 89, 120, 200)
LN2 = float(np.log(2.0))


def edge_logits():
    return np.array([(a, b) for a in EDGE_V for b in EDGE_V], dtype=np.float32)


def edge_classes(L):
    """(both dead, dead + live, weak, other) of the logit rows L.  Per logit: dead if l <= -89 (expf(-l) overflows,
    the sigmoid is exactly 0), band if -89 < l < -87 (the sigmoid is a float32 subnormal), live otherwise.  A row is
    weak if it has a band logit and both logits are below -60 or the other one is dead: what it scores depends on how
    subnormals are treated."""
    dead, band = L <= -89, (L > -89) & (L < -87)
    live = ~dead & ~band
    both_dead = dead.all(axis=1)
    low = (L < -60).all(axis=1)
    weak = (band[:, 0] & (low | dead[:, 1])) | (band[:, 1] & (low | dead[:, 0]))
    dead_live = (dead[:, 0] & live[:, 1]) | (dead[:, 1] & live[:, 0])
    assert not np.any(weak & both_dead) and not np.any(weak & dead_live) and not np.any(both_dead & dead_live)
    return both_dead, dead_live, weak, ~(both_dead | dead_live | weak)


def check_edge_rules(L, e):
    """The header's rules for etp on the rows L; returns the largest error of the "other" class."""
    e = np.asarray(e)
    both_dead, dead_live, weak, other = edge_classes(L)
    assert len(L) == 289 and both_dead.sum() == 9 and dead_live.sum() == 78
    assert weak.sum() <= 11                                     # the test leaves no more than these to either outcome
    assert np.all(np.isnan(e[both_dead]))                       # two sigmoids that underflow: 0 / 0
    assert np.all(e[dead_live] == 0) and not np.any(np.signbit(e[dead_live]))       # 0 log 0 = 0, -0 stored as +0
    w = e[weak]
    assert np.all(np.isnan(w) | ((w >= 0) & (w <= LN2 + ETP_TOL)))
    o = e[other]
    assert np.all(np.isfinite(o)) and not np.any(np.signbit(o))
    d = np.abs(o.astype(np.float64) - entropy64_of_logits(L[other]))
    assert d.max() <= ETP_TOL, float(d.max())
    return float(d.max())


def test_entropy_edge_rules_hold_for_the_float32_restatement():
    """The CPU twin of the device test below: scipy.stats.entropy of the float32 sigmoid 1 / (1 + exp(-l)), which is
    what PoolScorer(native=False) computes, obeys the same four rules on the same grid."""
    from scipy.stats import entropy
    L = edge_logits()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = np.float32(1) / (np.float32(1) + np.exp(-L))
        assert p.dtype == np.float32
        e = entropy(p, axis=1)
    assert edge_classes(L)[2].sum() == 11
    print("largest error of the ordinary rows", check_edge_rules(L, e))


@pytest.mark.gpu
def test_pool_entropy_edge_values():
    """NeuralNetCLS(2, 4, 2) with l = (relu(x0) - relu(-x0), relu(x1) - relu(-x1)): every product is by 0 or +-1, so
    the device logits are float32(x) bit for bit (which also pins k_pack's fragment packing at NT = 1), and the
    entropy epilogue is driven through its underflow, 0 log 0 and -0 branches."""
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    model = NeuralNetCLS(2, 4, 2)
    lin = [model.linear_relu_stack[i] for i in (0, 2, 4)]
    with torch.no_grad():
        lin[0].weight.copy_(torch.tensor([[1., 0.], [-1., 0.], [0., 1.], [0., -1.]]))
        lin[1].weight.copy_(torch.eye(4))
        lin[2].weight.copy_(torch.tensor([[1., -1., 0., 0.], [0., 0., 1., -1.]]))
        for l in lin:
            l.bias.zero_()
    model = model.cuda()
    L = edge_logits()
    X = L.astype(np.float64)
    sc = PoolScorer(1, model, None, "cuda")
    etp, lg = sc.entropy(sc.to_pool(X), 0.0, 1.0, logits=True)
    assert np.array_equal(lg.cpu().numpy().view(np.uint32), L.view(np.uint32))
    e = etp.cpu().numpy()
    weak = edge_classes(L)[2]
    assert weak.sum() == 11
    for row, v in zip(L[weak], e[weak]):
        print("weak row", row.tolist(), "etp", float(v))
    print("largest error of the ordinary rows", check_edge_rules(L, e))
    ref = PoolScorer(1, model, None, "cuda", native=False).entropy(X, 0.0, 1.0)
    assert np.array_equal(np.isnan(ref)[~weak], np.isnan(e)[~weak])


# -- 4., 5. the selection ---------------------------------------------------------------------------
def order_key(s):
    """The header's rule in numpy: NaN above every number (all NaNs tie), -0 equal to +0, subnormals ordered."""
    with np.errstate(invalid="ignore"):
        key = s.astype(np.float64)
    key[np.isposinf(s)] = 1e39
    key[np.isneginf(s)] = -1e39
    key[np.isnan(s)] = np.inf
    return key


def check_select(sc, s, sd, X, Xd, B, order):
    """One select call against `order`, the stable descending order of the scores: everything exact."""
    want = np.sort(order[:B])[::-1]
    r = sc.select(sd, Xd, B)
    tag = (len(s), B)
    assert np.array_equal(r["idx"], want), tag
    assert np.array_equal(r["X_sel"].cpu().numpy(), X[want]), tag
    keep = np.ones(len(s), dtype=bool)
    keep[want] = False
    assert np.array_equal(r["X_rest"].cpu().numpy(), X[keep]), tag
    assert np.array_equal(np.ascontiguousarray(r["scores"]).view(np.uint32), s[want].view(np.uint32)), tag
    if np.isnan(s[want]).any():
        assert np.isnan(r["etpmax"]), tag
    else:
        assert r["etpmax"] == float(s[want].max()), tag
    return r


def nin2_scorer():
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    return PoolScorer(1, NeuralNetCLS(2, 8, 2).cuda(), None, "cuda")


@functools.lru_cache(maxsize=None)
def pool2(n):
    """(X [n, 2] float64, the same on the device): the two-column pool of the selection tests; left unchanged."""
    X = np.random.default_rng(n).normal(size=(n, 2))
    return X, torch.from_numpy(X).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["distinct", "ties", "equal", "zeros"])
@pytest.mark.parametrize("n", [N_SEG2, N_SEG3])
def test_pool_selection_beyond_one_scan_segment(n, kind):
    """"equal" with B = n // 2 and "ties" put the cut between selected and unselected equal keys in the middle of the
    pool, where k_scan's running offE across the blocks of a segment decides which rows go where."""
    sc = nin2_scorer()
    s = _scores(kind, n, np.random.default_rng(n + len(kind)))
    X, Xd = pool2(n)
    sd = torch.from_numpy(s).cuda()
    order = np.argsort(-s, kind="stable")
    for B in (1, 46656, n // 2, n - 1, n):
        check_select(sc, s, sd, X, Xd, B, order)


SPECIALS = np.array([0x3F000000, 0xC0400000,                    # 0.5, -3
                     0x7F800000, 0xFF800000, 0x7F7FFFFF,        # +inf, -inf, FLT_MAX
                     0x00000001, 0x80000001,                    # 2^-149, -2^-149
                     0x00000000, 0x80000000,                    # +0, -0
                     0x7FC00000, 0xFFC00000, 0x7FA00001],       # NaN: quiet, sign bit set, another payload
                    dtype=np.uint32)


def special_scores(kind, n, rng):
    if kind == "negative":                                      # [-1, -2^-120], distinct: neighbours differ by 2^(120/n)
        s = -(2.0 ** (-120.0 * rng.permutation(n) / (n - 1))).astype(np.float32)
        assert len(np.unique(s)) == n and s.max() == -2.0 ** -120 and s.min() == -1.0
        return s
    bits = SPECIALS[rng.integers(0, len(SPECIALS), n)]          # chosen as integers: no float move touches a NaN
    assert len(np.unique(bits)) == len(SPECIALS)
    return bits.view(np.float32)


def test_the_reference_order_of_special_scores():
    s = SPECIALS.view(np.float32)
    assert s[0] == 0.5 and s[1] == -3.0 and s[4] == np.finfo(np.float32).max and s[5] == 2.0 ** -149 == -s[6]
    assert np.isnan(s[9:]).all() and np.signbit(s[10]) and np.signbit(s[8]) and not np.signbit(s[7])
    order = np.argsort(-order_key(s), kind="stable")
    #        NaNs by index | +inf FLT_MAX 0.5 2^-149 | the zeros by index | -2^-149 -3 -inf
    assert order.tolist() == [9, 10, 11, 2, 4, 0, 5, 7, 8, 6, 1, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["negative", "specials"])
@pytest.mark.parametrize("n", [1000, 70001])
def test_pool_selection_on_special_scores(n, kind):
    sc = nin2_scorer()
    s = special_scores(kind, n, np.random.default_rng(n + len(kind)))
    X, Xd = pool2(n)
    sd = torch.from_numpy(s).cuda()
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), s.view(np.uint32))
    order = np.argsort(-order_key(s), kind="stable")
    for B in (1, 37, n // 2, n):
        r = check_select(sc, s, sd, X, Xd, B, order)
        if kind == "negative":
            assert r["etpmax"] == -2.0 ** -120                  # a negative maximum


# -- 6. scratch buffers on a live handle, the index-only call, argument errors ------------------------
@pytest.mark.gpu
def test_pool_select_regrows_its_counters_on_a_live_handle():
    sc = nin2_scorer()
    for n in (1000, 70001, N_SEG2, 1000):
        s = _scores("ties", n, np.random.default_rng(n + 4))
        X, Xd = pool2(n)
        check_select(sc, s, torch.from_numpy(s).cuda(), X, Xd, 37, np.argsort(-s, kind="stable"))


def guess_bound(g, X0, mean, std, hidden):
    """(float64 stages 1..N [B, nin N], bound) as test_pool_guess_matches_float64_forward_and_nn_guess derives them."""
    nin = X0.shape[1]
    out, a3 = forward64(params64(g), norm32(X0, mean, std))
    c = nin + 2 * padded(hidden) + 3
    return out * np.float64(np.float32(std)) + np.float64(np.float32(mean)), U * ((c + 2) * a3 * std + abs(mean))


@pytest.mark.gpu
def test_pool_guess_regrows_its_hidden_buffer_on_a_live_handle():
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    nin, hidden, N = 6, 500, 100
    torch.manual_seed(11)
    g = NeuralNetCLS(nin, hidden, nin * N).cuda()
    cls = NeuralNetCLS(nin, hidden, 2).cuda()
    mean, std = float(np.float32(1.3)), float(np.float32(5.1))
    live = PoolScorer(3, cls, g, "cuda")
    for B in (3, 300, 17):
        X0 = pool_rows(nin, B, seed=B)
        got = live.guess(X0, N, mean, std)
        fresh = PoolScorer(3, cls, g, "cuda").guess(X0, N, mean, std)
        assert got.shape == (B, N + 1, nin) and torch.equal(got, fresh), B


@pytest.mark.gpu
def test_pool_guess_network_changes_its_outputs_on_a_live_handle():
    from vboc_amd.learn import NeuralNetCLS, PoolScorer
    nin, hidden, B = 6, 64, 33
    torch.manual_seed(12)
    cls = NeuralNetCLS(nin, hidden, 2).cuda()
    nets = {N: NeuralNetCLS(nin, hidden, nin * N).cuda() for N in (5, 100)}
    mean, std = float(np.float32(1.3)), float(np.float32(5.1))
    X0 = pool_rows(nin, B, seed=B)
    live = PoolScorer(3, cls, nets[5], "cuda")
    for N in (5, 100, 5):                                       # O = 30 (OP 64), 600 (OP 640), 30
        live.guess_model = nets[N]
        got = live.guess(X0, N, mean, std)
        fresh = PoolScorer(3, cls, nets[N], "cuda").guess(X0, N, mean, std)
        assert got.shape == (B, N + 1, nin) and torch.equal(got, fresh), N
        h = got.cpu().numpy()
        assert np.array_equal(h[:, 0], X0)
        want, bound = guess_bound(nets[N], X0, mean, std, hidden)
        assert np.all(np.abs(h[:, 1:].reshape(B, -1) - want) <= bound), N


@pytest.mark.gpu
@pytest.mark.parametrize("B", [37, 35000])
def test_pool_select_without_the_pool(B):
    """X = NULL: the indices alone, equal to those of the call that also compacts X."""
    from vboc_amd import poollib
    n = 70001
    sc = nin2_scorer()
    s = _scores("ties", n, np.random.default_rng(n))
    X, Xd = pool2(n)
    sd = torch.from_numpy(s).cuda()
    r = sc.select(sd, Xd, B)
    idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    mx = ctypes.c_float(-1.0)
    poollib.check(poollib.load().vboc_pool_select(sc._h, sd.data_ptr(), None, n, B, 2, idx.data_ptr(), None, None,
                                                  ctypes.byref(mx), torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(idx.cpu().numpy(), r["idx"]) and mx.value == r["etpmax"] == float(s.max())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1 << 31, -1])
def test_pool_row_counts_outside_the_range_are_refused(n):
    from vboc_amd import poollib
    sc = nin2_scorer()
    lib = poollib.load()
    st = torch.cuda.current_stream().cuda_stream
    etp = torch.zeros(4, device="cuda")
    X = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    sc.entropy(X, 0.0, 1.0)                                     # the classifier is set: only n is wrong below
    assert lib.vboc_pool_entropy(sc._h, X.data_ptr(), n, 0.0, 1.0, etp.data_ptr(), None, None, st) == poollib.EARG
    assert b"2^31" in lib.vboc_pool_last_error()
    mx = ctypes.c_float(-1.0)
    assert lib.vboc_pool_select(sc._h, etp.data_ptr(), X.data_ptr(), n, 1 if n > 0 else 0, 2, idx.data_ptr(),
                                X.data_ptr(), X.data_ptr(), ctypes.byref(mx), st) == poollib.EARG
    assert b"2^31" in lib.vboc_pool_last_error() and mx.value == -1.0
    torch.cuda.synchronize()
    assert not etp.any() and not idx.any()
