"""The certificate of the digit-slice scan against its restatement (tests/cert_truth.py, pinned on the CPU by tests/test_cert_host.py).

(a) The block kernels (eagle_dev_cert_lb_b / _select_b / _accumulate; csrc/eagle_i8mfma.hip) on fabricated arrays: they read a, vara, bound
and the two budgets at the head of the digit workspace and nothing else, so no scan is needed.  Every figure is compared with `==`: the
bits of the lower bound, over_tight, flagged, count, overflow and the sorted index list -- at lengths on both sides of a block, of the
2,048 x 256 grid (the second trip of the stride loop) and beyond, with rows planted on every skip and on both knife edges, at 2,048 and
2,049 qualifying rows and with 512 and 513 markers over the tight threshold.

(b) The one-block flow (eagle_dev_scan_certify_lb / _apply, bounds recomputed inline) against the block flow (eagle_dev_cert_bounds once,
then _lb_b / _select_b) on the state a real scan leaves behind, in five states of the bound; the bound itself against cert_truth.bound_of;
and both caps through the gated path that ships: which rows hold the fp64 kernel's bits afterwards."""
import ctypes as C

import numpy as np
import pytest

import cert_truth as ct
import exact_lastdigit as xl

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 255, 256, 257, 524288, 524289, 1000003)


@pytest.fixture(scope="module")
def api():
    from eagleeverything_amd import rcpp_api
    assert rcpp_api.device_info()["arch"].startswith("gfx950")
    yield rcpp_api
    rcpp_api.close_all()


class Block:
    """The block flow on host arrays: one cert_ws, one 256-byte stand-in for the head of the digit workspace."""

    def __init__(self, api, budget=ct.TIGHT, budget_loose=ct.LOOSE):
        import torch
        from eagleeverything_amd import _lib
        self.torch, self.L, self.ctx = torch, _lib.load(), api.context(0)
        self.dev = torch.device("cuda", 0)
        self.cert_ws = torch.zeros(int(self.L.eagle_scan_certify_workspace_bytes(256)), dtype=torch.uint8, device=self.dev)
        self.vara_ws = torch.from_numpy(ct.fabricated_header(budget, budget_loose)).to(self.dev)
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def check(self, rc):
        assert rc == 0, self.L.eagle_last_error(self.ctx).decode()

    def load(self, case):
        up = lambda x: self.torch.from_numpy(np.ascontiguousarray(x if len(x) else np.zeros(1), dtype=np.float64)).to(self.dev)
        self.n = len(case["a"])
        self.a, self.vara, self.bound = up(case["a"]), up(case["vara"]), up(case["bound"])

    def head(self):
        self.torch.cuda.synchronize()
        h = self.cert_ws[:24].cpu().numpy().tobytes()
        i = np.frombuffer(h[8:24], dtype=np.int32)
        return dict(lb_bits=int(np.frombuffer(h[:8], dtype=np.uint64)[0]), lower_bound=float(np.frombuffer(h[:8], dtype=np.float64)[0]),
                    count=int(i[0]), overflow=int(i[1]), flagged=int(i[2]), tight=int(i[3]))

    def indices(self, count):
        k = min(count, ct.CERT_CAP)
        return np.sort(np.frombuffer(self.cert_ws[256:256 + 8 * k].cpu().numpy().tobytes(), dtype=np.int64))

    def lower_bound(self):
        self.check(self.L.eagle_dev_cert_lb_b(self.ctx, self.n, self.a.data_ptr(), self.vara.data_ptr(), self.bound.data_ptr(),
                                              self.cert_ws.data_ptr(), self.vara_ws.data_ptr(), self.stream))
        return self.head()

    def select(self, lb, over_tight):
        self.check(self.L.eagle_dev_cert_select_b(self.ctx, self.n, self.a.data_ptr(), self.vara.data_ptr(), self.bound.data_ptr(),
                                                  self.cert_ws.data_ptr(), float(lb), int(over_tight), self.vara_ws.data_ptr(), self.stream))
        return self.head()

    def run(self, case, lb=None, over_tight=None, what=""):
        """lb_b then select_b (lb / over_tight: None = the block's own) against cert_truth.predict, every figure with ==."""
        want = ct.predict(case, lb, over_tight)
        self.load(case)
        h = self.lower_bound()
        assert h["lb_bits"] == int(np.float64(want["lower_bound"]).view(np.uint64)), (what, h["lower_bound"], want["lower_bound"])
        assert h["tight"] == want["over_tight"] and (h["count"], h["overflow"], h["flagged"]) == (0, 0, 0), (what, h, want["over_tight"])
        g = self.select(h["lower_bound"] if lb is None else lb, h["tight"] if over_tight is None else over_tight)
        sel = want["sel"]
        print("%s: restatement lb %r tight %d count %d flagged %d overflow %d | device lb %r tight %d count %d flagged %d overflow %d"
              % (what, want["lower_bound"], want["over_tight"], sel.count, sel.flagged, sel.overflow, g["lower_bound"], g["tight"], g["count"],
                 g["flagged"], g["overflow"]))
        assert (g["count"], g["flagged"], g["overflow"], g["tight"], g["lb_bits"]) == (sel.count, sel.flagged, sel.overflow, want["over_tight"],
                                                                                       h["lb_bits"]), (what, g, sel[1:])
        if sel.count <= ct.CERT_CAP:
            assert np.array_equal(self.indices(g["count"]), sel.idx), (what, self.indices(g["count"])[:8], sel.idx[:8])
        else:                                                            # the 2,048 it kept are rows that qualify, each once
            kept = self.indices(g["count"])
            assert kept.size == ct.CERT_CAP == np.unique(kept).size and np.isin(kept, sel.idx).all(), what
        return g


@pytest.fixture(scope="module")
def block(api):
    return Block(api)


def test_tight_max_is_the_restated_one(block):
    assert block.L.eagle_cert_tight_max() == ct.CERT_TIGHT_MAX
    off = block.L.eagle_cert_indices(block.cert_ws.data_ptr()) - block.cert_ws.data_ptr()
    rows = block.L.eagle_cert_rows(block.cert_ws.data_ptr()) - block.cert_ws.data_ptr()
    assert (off, rows) == (256, 256 + 8 * ct.CERT_CAP)


@pytest.mark.parametrize("L", LENGTHS)
def test_block_kernels_on_planted_rows(block, L):
    """Skips (NaN, +Inf, -Inf in a and in vara; vara + b = 0; vara < 0), vara - b = 0 and < 0, a = 0, b = 0, and both knife edges
    (b == 1.8 budget |vara|: not flagged, one unit in the last place above: flagged; (a*a)/(vara-b) == thr: a candidate, one below: not)
    from index 0, from L - 1 and on both sides of marker 524,288 -- against the block's own lower bound, against a larger one handed in (the
    multi-device case, its threshold on the knife edge) and against lb = 0, where every finite row qualifies."""
    case = ct.edge_case(L)
    own = block.run(case, what="L=%d own lb" % L)
    assert L == 0 or own["lower_bound"] > 0.0
    block.run(case, lb=ct.lb_with_threshold(np.float64(ct.EDGE_Q)), what="L=%d lb on the knife edge" % L)
    g = block.run(case, lb=0.0, what="L=%d lb=0" % L)
    assert g["overflow"] == int(g["count"] > ct.CERT_CAP)
    # a larger lower bound with nothing special about it, and the tier switch on the same rows
    block.run(case, lb=1.5 * ct.PEAK, over_tight=ct.CERT_TIGHT_MAX + 1, what="L=%d lb=384, default budget enforced" % L)


@pytest.mark.parametrize("L", [524288, 524289, 1000003])
def test_block_kernels_at_the_candidate_cap(block, L):
    """Exactly 2,048 qualifying rows: overflow 0 and every index present; 2,049: overflow 1."""
    for k in (ct.CERT_CAP, ct.CERT_CAP + 1):
        case = ct.cap_case(L, k)
        want = ct.predict(case)["sel"]
        assert (want.count, want.overflow) == (k, int(k > ct.CERT_CAP))
        g = block.run(case, what="L=%d %d qualifying rows" % (L, k))
        assert (g["count"], g["overflow"]) == (k, int(k > ct.CERT_CAP))


@pytest.mark.parametrize("L", [257, 1000003])
def test_block_kernels_at_the_tier_switch_and_accumulate(block, L):
    """Rows with b = 3e-7 |vara| (between 1.8 x 1e-7 and 1.8 x 5e-7): with 512 markers of the whole scan over the tight threshold they are
    all flagged, with 513 none is.  Then eagle_dev_cert_accumulate twice into four zeroed longs."""
    m = 100 if L < 1000 else 700
    case = ct.tier_case(L, m)
    assert ct.predict(case, over_tight_all=512)["sel"].flagged == m and ct.predict(case, over_tight_all=513)["sel"].flagged == 0
    g = block.run(case, over_tight=ct.CERT_TIGHT_MAX + 1, what="L=%d tier, 513 over" % L)
    assert (g["flagged"], g["count"], g["tight"]) == (0, 1, m)
    g = block.run(case, over_tight=ct.CERT_TIGHT_MAX, what="L=%d tier, 512 over" % L)
    assert (g["flagged"], g["count"], g["tight"]) == (m, m + 1, m)
    for case2, g2 in ((case, g), (ct.cap_case(max(L, 4096), ct.CERT_CAP + 1), None)):
        if g2 is None:
            g2 = block.run(case2, what="accumulate after an overflow")
        totals = block.torch.zeros(4, dtype=block.torch.int64, device=block.dev)
        for _ in range(2):
            block.check(block.L.eagle_dev_cert_accumulate(block.ctx, block.cert_ws.data_ptr(), totals.data_ptr(), block.stream))
        block.torch.cuda.synchronize()
        assert totals.cpu().tolist() == [2 * min(g2["count"], ct.CERT_CAP), 2 * g2["flagged"], 2 * g2["overflow"], 2 * g2["tight"]]


def test_block_lower_bound_when_a_square_overflows(block):
    """a^2 = +Inf for one marker.  Not an equality: the device looks at finiteness after a wave of 64 has been reduced, so the wave that
    holds the marker contributes nothing -- here the finite maximum (row 100) goes with it and the bound comes from row 300.  Lower, and
    still a lower bound; the marker itself is selected whatever the bound."""
    case = ct.inf_case()
    want = ct.predict(case)
    block.load(case)
    h = block.lower_bound()
    print("a^2 overflows: restatement's maximum over the finite terms %r, device %r" % (want["lower_bound"], h["lower_bound"]))
    assert np.isfinite(h["lower_bound"]) and 0.0 <= h["lower_bound"] <= want["lower_bound"]
    g = block.select(h["lower_bound"], h["tight"])
    idx = block.indices(g["count"])
    assert 70 in idx.tolist() and g["overflow"] == 0
    assert np.array_equal(idx, ct.select(case["a"], case["vara"], case["bound"], h["lower_bound"], case["budget"], case["budget_loose"], h["tight"]).idx)


# ---- (b) the two flows on a real scan state -------------------------------------------------------------------------------------------------
N, LM = 300, 3000                     # 12 column tiles of markers, one 256-tile of individuals with padding (n_pad = 512), L_pad = 3,072
LB0 = 100.0
STATES = ("default", "tight", "slices3", "stochastic", "spectral_ext", "w8")
# default: the shipped path (here: two digits under the level-2 spectral bound, which holds the default budget only); tight: the saving
# switched off -- three digits, n_pad^2 2^(e+1-24) = 1.22e-4 <= 1e-7 sum_k |W_kk| / 2 = 2.4e-4: the tight budget in force with the default
# behind it; slices3: the digit count forced; stochastic: the Hoeffding radius; spectral_ext: the last digit dropped and given back to the
# markers that fail their budget (extension flags set); w8: W from the int8 engine (wErr > 0)


def _r256(x):
    return (x + 255) // 256 * 256


class Scan:
    """A DeviceShard after one uncertified digit-slice scan in one state of the bound, and everything bound_of needs, on the host."""

    def __init__(self, api, state, n=N, L=LM, host_rows=None):
        import torch
        from eagleeverything_amd.sharded import DeviceShard
        self.torch, self.state, self.n, self.Lm = torch, state, n, L
        sh = self.sh = DeviceShard(n, L)
        assert (n, L) != (N, LM) or (sh.np_, sh.Lp) == (512, 3072)
        N_, LM_ = n, L
        if state == "spectral_ext":       # the last digit chosen so that level 2 takes it off and the markers on the quiet individuals fail their budget
            case = xl.build_case(N_, LM_, 4, state="l2", quiet=32, adversarial=6)
            sh.Mt8[:LM_, :N_] = torch.from_numpy(case["Mt8"].copy()).to(sh.dev)
            S, V, ahat = case["S"], case["V"], case["ahat"]
        else:                             # off-diagonal ~1e-3, diagonal ~20: the tight budget is in force on three digits
            sh.fill_synthetic(seed=31)
            gen = torch.Generator(device=sh.dev)
            gen.manual_seed(9)
            E = torch.randn((N_, N_), generator=gen, device=sh.dev, dtype=torch.float64) * 1e-3
            V = torch.diag(20.0 * (0.8 + 0.4 * torch.rand(N_, generator=gen, device=sh.dev, dtype=torch.float64))) + 0.5 * (E + E.T)
            S = 0.9 * torch.eye(N_, dtype=torch.float64, device=sh.dev)
            ahat = torch.randn(N_, generator=gen, device=sh.dev, dtype=torch.float64)
        sh.set_operands(S, V, ahat)
        sh._check(sh.L.eagle_set_scan_budget(sh.ctx, 0.0))               # the default policy: 1e-7 first, then 5e-7
        sh.L.eagle_dev_set_spectral(sh.ctx, 0 if state == "tight" else 1)
        sh.mode, sh.certified = 1, False
        sh.nslices = 3 if state == "slices3" else 0
        sh.stochastic = state == "stochastic"
        sh.w_mode = 2 if state == "w8" else 1
        sh.scan()
        torch.cuda.synchronize()
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
        self.raw_a, self.raw_vara = sh.a.clone(), sh.vara.clone()
        self.hdr = xl.decode_header(sh.ws[:256].cpu().numpy())
        l1 = sh.l1[:LM_].cpu().numpy().astype(np.int64)
        self.l1, self.q2 = l1[:, 0], l1[:, 1]
        self.c = sh.cshift[:LM_].cpu().numpy().astype(np.int64)
        # the extension's flags: [slice slots | 256 B | idx: 4 cap | flag: L_pad | ...] behind the slots, and counted from the end as well
        ns, nslots = sh._ns(), C.c_int(0)
        cap = (min(sh.Lp, 65536) + 767) // 768 * 768
        off = _r256(int(sh.L.eagle_vara_i8_ws_slot_offset(sh.np_, sh.Lp, ns, 0, C.byref(nslots))) + nslots.value * sh.np_ * sh.np_) + 256 + _r256(4 * cap)
        assert off == int(sh.L.eagle_vara_i8_workspace_bytes(sh.np_, sh.Lp, ns)) - cap * sh.np_ - _r256(8 * cap) - _r256(sh.Lp) and sh.ws.numel() >= off + sh.Lp
        self.ext = sh.ws[off:off + LM_].cpu().numpy() != 0
        # the diagonal term and m^T rho in fp64 on the host from the folded W (rho_j = sum_{k>j} Wu_jk + sum_{k<j} Wu_kj)
        Wu = sh.Wu.cpu().numpy()
        self.hrows = np.arange(LM_) if host_rows is None else np.asarray(host_rows, dtype=np.int64)     # the rows the host recomputes
        M = sh.Mt8[torch.from_numpy(self.hrows).to(sh.dev)].cpu().numpy().astype(np.float64)
        up = np.triu(Wu, 1)
        rho, rho_abs = up.sum(axis=1) + up.sum(axis=0), np.abs(up).sum(axis=1) + np.abs(up).sum(axis=0)
        if state == "w8":   # W from the int8 engine: the library takes rho from r = S (V (S 1)) in fp64, not from this image; read it, and hold it to the image
            roff = int(sh.L.eagle_vara_i8_ws_rowsum_offset(sh.np_, sh.Lp, ns)) - 8 * sh.np_
            rho_dev = np.frombuffer(sh.ws[roff:roff + 8 * sh.np_].cpu().numpy().tobytes(), dtype=np.float64)
            assert np.all(np.abs(rho_dev - rho) <= 2.0 * (np.sqrt(sh.np_) + 1.0) * self.hdr["wErr"] + 1e-10 * rho_abs)
            rho = rho_dev
        d = np.diag(Wu)
        self.vdiag, self.vd_abs = (M * M) @ d, (M * M) @ np.abs(d)
        self.mrho, self.mr_abs = M @ rho, np.abs(M) @ rho_abs
        self.cert_ws = torch.zeros(int(sh.L.eagle_scan_certify_workspace_bytes(sh.np_)), dtype=torch.uint8, device=sh.dev)
        sh.cert_ws = self.cert_ws
        self.bound = torch.zeros(sh.Lp, dtype=torch.float64, device=sh.dev)
        self.block = Block.__new__(Block)
        self.block.__dict__.update(torch=torch, L=sh.L, ctx=sh.ctx, dev=sh.dev, cert_ws=self.cert_ws, vara_ws=sh.ws, stream=sh._stream(), n=LM_,
                                   a=sh.a, vara=sh.vara, bound=self.bound)

    def bounds(self):
        sh = self.sh
        sh._check(sh.L.eagle_dev_cert_bounds(sh.ctx, self.Lm, sh.Lp, sh.np_, sh.cshift.data_ptr(), sh.l1.data_ptr(), sh._ns(), sh.ws.data_ptr(),
                                             sh.vara.data_ptr(), self.bound.data_ptr(), sh._stream()))
        self.torch.cuda.synchronize()
        return self.bound[:self.Lm].cpu().numpy()

    def host(self):
        return self.sh.a[:self.Lm].cpu().numpy(), self.sh.vara[:self.Lm].cpu().numpy()

    def put(self, a=None, vara=None):
        for dst, src in ((self.sh.a, a), (self.sh.vara, vara)):
            if src is not None:
                dst[:self.Lm] = self.torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64)).to(self.sh.dev)

    def restore(self):
        self.sh.a.copy_(self.raw_a)
        self.sh.vara.copy_(self.raw_vara)

    def plant(self, rows, vara, b):
        """a such that exactly `rows` are candidates by rule (2) whatever LB turns out to be: a_i^2 = LB0 (vara_i - b_i) (1 + 1e-6) for
        them, half of LB0 (vara_i - b_i) for everybody else (LB = max a^2 / (vara + b) lies a few b / vara under LB0 (1 + 1e-6)).  A row
        without an upper bound (vara_i - b_i <= 0: it qualifies on its own) gets a = 0."""
        scale = np.full(self.Lm, 0.5)
        scale[rows] = 1.0 + 1e-6
        den = vara - b
        return np.where(den > 0.0, np.sqrt(LB0 * np.where(den > 0.0, den, 1.0) * scale), 0.0)

    def one_block(self, lb_override=np.nan):
        """eagle_dev_scan_certify_lb, then _apply -> (head after _lb, head after _apply, sorted indices)."""
        sh, blk = self.sh, self.block
        sh._check(sh.L.eagle_dev_scan_certify_lb(sh.ctx, self.Lm, sh.Lp, sh.np_, sh.cshift.data_ptr(), sh.l1.data_ptr(), sh._ns(), sh.ws.data_ptr(),
                                                 sh.a.data_ptr(), sh.vara.data_ptr(), self.cert_ws.data_ptr(), sh._stream()))
        h = blk.head()
        sh._check(sh.L.eagle_dev_scan_certify_apply(sh.ctx, sh.Mt8.data_ptr(), self.Lm, sh.Lp, sh.np_, sh.np_, sh.cshift.data_ptr(), sh.l1.data_ptr(),
                                                    sh._ns(), sh.ws.data_ptr(), sh.Wu.data_ptr(), sh.a.data_ptr(), sh.vara.data_ptr(),
                                                    self.cert_ws.data_ptr(), float(lb_override), sh._stream()))
        g = blk.head()
        return h, g, blk.indices(g["count"])


def _away_from_the_flag_edges(vara, b, hdr):
    for budget in (hdr["budget"], hdr["budget_loose"]):
        with np.errstate(all="ignore"):
            r = b / (ct.FLAG_FACTOR * budget * np.abs(vara))
        assert not np.any(np.abs(r - 1.0) < 1e-6)


@pytest.mark.parametrize("state", STATES)
def test_bound_and_both_flows_on_a_real_scan_state(api, state):
    """eagle_dev_cert_bounds against cert_truth.bound_of, then the one-block flow against the block flow and the restatement.

    The tolerance of the bound.  Host and device evaluate the same expression in fp64: the leading term (up to three products and a
    minimum), wErr q2, 2^-48 mag and 2^-50 sumdiag, all non-negative, summed left to right -- at most 8 roundings on either side (fewer on
    the device where a product is contracted into the sum), each relative to a partial sum that is at most b: 16 x 2^-53 b.  mag itself is
    fed from the diagonal term and m^T rho, which host and device sum in different orders: either is off by at most gamma sum_k m_k^2 |W_kk|
    resp. gamma sum_j |m_j| (sum_k |Wu_jk| + |Wu_kj|), gamma = 2 n_pad 2^-53 (rho's own sum and the product with m); the diagonal term
    enters mag twice, m^T rho with a factor 2, both sides count: 2^-48 x 2 gamma (2 vd_abs + 2 mr_abs).  R, sumdiag, specH, wErr, e, S come
    from the decoded header, l1, q2 and c from the device's own integers: no error."""
    sc = Scan(api, state)
    sh, hdr = sc.sh, sc.hdr
    print(state, {k: hdr[k] for k in ("S", "S_sliced", "pad", "e", "specH", "wErr", "budget", "budget_loose", "level", "sumdiag", "R")},
          "extended", int(sc.ext.sum()), "c != 0", int((sc.c != 0).sum()))
    assert hdr["maxabs_off"] > 0.0
    if state == "slices3":
        assert (hdr["S"], hdr["specH"], hdr["pad"]) == (3, 0.0, 0)
    if state == "tight":
        assert (hdr["S"], hdr["specH"], hdr["budget"], hdr["budget_loose"]) == (3, 0.0, ct.TIGHT, ct.LOOSE)
    if state == "stochastic":
        assert hdr["pad"] == 1 and hdr["specH"] == 0.0
    if state == "spectral_ext":
        assert hdr["specH"] > 0.0 and hdr["S_sliced"] == hdr["S"] + 1 and 0 < sc.ext.sum() < LM
    else:
        assert not sc.ext.any() or hdr["specH"] > 0.0
    if state == "w8":
        assert hdr["wErr"] > 0.0 and sh.w_info()["int8"] == 1
    else:
        assert hdr["wErr"] == 0.0
    assert (sc.c != 0).any()
    b_dev, v0 = _assert_bound(sc)
    # planted candidates: rows next to the tile edges and seeded ones; then the flows
    rows = np.union1d(ct.spread(LM, 37, seed=len(state)), [1, 254, 257, 2815, 2816, 2998])
    for override in (None, 1.0001, 0.0):
        _assert_flows(sc, rows, v0, b_dev, override)


def _assert_bound(sc):
    """eagle_dev_cert_bounds on the state as it is against bound_of on the rows the host recomputed -> (device bounds, vara)."""
    sh, hdr, hr = sc.sh, sc.hdr, sc.hrows
    b_dev = sc.bounds()
    _, v0 = sc.host()
    want = ct.bound_of(hdr, sc.l1[hr], sc.q2[hr], sc.c[hr], sc.vdiag, sc.mrho, v0[hr], sc.ext[hr])
    gamma = 2.0 * sh.np_ * 2.0 ** -53
    tol = 16 * 2.0 ** -53 * want + 2.0 ** -48 * 2.0 * gamma * (2.0 * sc.vd_abs + 2.0 * sc.mr_abs)
    worst = float((np.abs(b_dev[hr] - want) / tol).max())
    with np.errstate(all="ignore"):
        rel = b_dev / np.abs(v0)
    print(sc.state, "bound: largest |device - restatement| / tolerance %.3g, b / |vara| in [%.3g, %.3g]" % (worst, rel.min(), rel.max()))
    assert np.all(b_dev > 0.0) and np.all(np.abs(b_dev[hr] - want) <= tol), worst
    _away_from_the_flag_edges(v0, b_dev, hdr)
    return b_dev, v0


def _assert_flows(sc, rows, v0, b_dev, override):
    """`rows` planted as candidates, then lb_b / select_b and scan_certify_lb / _apply against the restatement and each other.
    override: None = the block's own lower bound; a factor above 1 = that multiple of it handed in (the multi-device case: the planted
    rows fall out); 0.0 = lb = 0 handed in with a = 0 planted on five rows: every finite row qualifies, and 0 / (vara - b) >= 0 is the
    comparison's equality without any rounding of b in it (more than 2,048: overflow, where the count still tells)."""
    hdr, state, Lm = sc.hdr, sc.state, sc.Lm
    own_way = ~(v0 - b_dev > 0.0) | (b_dev > ct.FLAG_FACTOR * hdr["budget"] * np.abs(v0))       # rows that qualify whatever a is
    rows = rows[~own_way[rows]]
    assert rows.size >= 6
    sc.restore()
    a1 = sc.plant(rows, v0, b_dev)
    if override == 0.0:
        a1[rows[:5]] = 0.0
    sc.put(a=a1)
    a1, _ = sc.host()
    own = ct.lower_bound(a1, v0, b_dev)
    lb = own if override is None else override * own
    tight = ct.over_tight(v0, b_dev, hdr["budget"], a1)
    sel = ct.select(a1, v0, b_dev, lb, hdr["budget"], hdr["budget_loose"], tight)
    natural = np.setdiff1d(sel.idx, rows)
    if override is None:
        assert np.isin(rows, sel.idx).all() and sel.count == rows.size + natural.size and sel.overflow == 0
        assert 0.0 < own <= LB0 * (1 + 1e-6)
    elif override == 0.0:
        assert sel.count == Lm and sel.overflow == int(Lm > ct.CERT_CAP) and (a1 == 0.0).sum() >= 5
    else:
        assert not np.isin(rows, sel.idx).any()
    # nobody within 1e-10 of the threshold (the planted rows are tied at or above LB, so the slack alone leaves them 1e-9): the two
    # flows may round b differently in its last place, which moves a quotient by 1e-16 b / vara
    thr = ct.thr_of(lb)
    with np.errstate(all="ignore"):
        q = (a1 * a1) / (v0 - b_dev)
    assert thr == 0.0 or not np.any(np.abs(q / thr - 1.0) < 1e-10)
    hb = sc.block.lower_bound()
    gb = sc.block.select(lb, hb["tight"])
    ib = sc.block.indices(gb["count"])
    h1, g1, i1 = sc.one_block(np.nan if override is None else lb)
    print("%s override %r: restatement lb %r tight %d count %d flagged %d | block flow lb %r tight %d count %d flagged %d | one-block flow lb %r "
          "tight %d count %d flagged %d" % (state, override, own, tight, sel.count, sel.flagged, hb["lower_bound"], hb["tight"], gb["count"],
                                           gb["flagged"], h1["lower_bound"], h1["tight"], g1["count"], g1["flagged"]))
    assert hb["lb_bits"] == int(np.float64(own).view(np.uint64)) and hb["tight"] == tight
    assert (h1["lb_bits"], h1["tight"]) == (hb["lb_bits"], hb["tight"])
    for g, i in ((gb, ib), (g1, i1)):
        assert (g["count"], g["flagged"], g["overflow"]) == (sel.count, sel.flagged, sel.overflow)
        if sel.overflow:
            assert i.size == ct.CERT_CAP == np.unique(i).size and np.isin(i, sel.idx).all()
        else:
            assert np.array_equal(i, sel.idx)
    sc.restore()


def test_one_block_flow_on_the_second_grid_trip(api):
    """k_cert_bounds, k_cert_lb and k_cert_select with more than 2,048 x 256 markers in front of them: n = 100, L = 524,300.  The bound
    is held to bound_of on the rows from 524,282 on (a thread that left after its first trip would leave zeros there), candidates are
    planted at both ends and on both sides of marker 524,288."""
    L = ct.ONE_TRIP + 12
    sc = Scan(api, "tight", n=100, L=L, host_rows=np.arange(ct.ONE_TRIP - 6, L))
    assert sc.sh.np_ == 256 and sc.sh.Lp > ct.ONE_TRIP and sc.hdr["specH"] == 0.0
    b_dev, v0 = _assert_bound(sc)
    rows = np.array([0, 255, 256, ct.ONE_TRIP - 2, ct.ONE_TRIP - 1, ct.ONE_TRIP, ct.ONE_TRIP + 1, L - 2, L - 1])
    _assert_flows(sc, rows, v0, b_dev, None)


@pytest.fixture(scope="module")
def gated(api):
    """The state with the tight budget in force, its mode-0 values (eagle_dev_vara_f64) and its device bounds, shared by the cap tests below."""
    sc = Scan(api, "tight")
    sh = sc.sh
    sh.mode = 0
    sh.scan()
    sc.torch.cuda.synchronize()
    v64 = sh.vara[:LM].clone()
    sh.mode = 1
    sc.restore()
    assert sc.hdr["wErr"] == 0.0 and not sc.torch.equal(v64, sc.raw_vara[:LM])
    return sc, v64


def _certify(sc):
    sc.sh.certify()
    sc.torch.cuda.synchronize()
    info = sc.sh.certificate()
    k = min(sc.block.head()["count"], ct.CERT_CAP)
    return info, sc.block.indices(k)


def test_candidate_cap_through_the_gated_path(gated):
    """2,048 qualifying markers: overflow 0, exactly those rows hold the bits of the mode-0 scan and every other row its raw digit value.
    2,049: overflow 1 and all rows hold the mode-0 bits."""
    sc, v64 = gated
    torch = sc.torch
    for k in (ct.CERT_CAP, ct.CERT_CAP + 1):
        sc.restore()
        _, v0 = sc.host()
        b = sc.bounds()
        probe = ct.select(sc.plant(np.array([0]), v0, b), v0, b, LB0, sc.hdr["budget"], sc.hdr["budget_loose"],
                          ct.over_tight(v0, b, sc.hdr["budget"]))
        natural = np.setdiff1d(probe.idx, [0])                            # rows that qualify on their own (flagged, or no upper bound)
        rows = ct.spread(LM, k, seed=k)
        rows = np.setdiff1d(rows, natural)[:k - natural.size] if natural.size else rows
        a1 = sc.plant(rows, v0, b)
        sc.put(a=a1)
        want = ct.select(a1, v0, b, ct.lower_bound(a1, v0, b), sc.hdr["budget"], sc.hdr["budget_loose"], ct.over_tight(v0, b, sc.hdr["budget"], a1))
        assert want.count == k and want.overflow == int(k > ct.CERT_CAP)
        info, idx = _certify(sc)
        print("gated path, %d qualifying: restatement count %d flagged %d overflow %d | device %r" % (k, want.count, want.flagged, want.overflow, info))
        assert info["overflow"] == want.overflow and info["flagged"] == want.flagged and info["reevaluated"] == ct.CERT_CAP
        got = sc.sh.vara[:LM]
        if k == ct.CERT_CAP:
            assert np.array_equal(idx, want.idx)
            mask = torch.zeros(LM, dtype=torch.bool, device=sc.sh.dev)
            mask[torch.from_numpy(want.idx).to(sc.sh.dev)] = True
            assert torch.equal(got[mask], v64[mask]) and torch.equal(got[~mask], sc.raw_vara[:LM][~mask])
            assert not torch.equal(got[mask], sc.raw_vara[:LM][mask])
        else:
            assert torch.equal(got, v64)
    sc.restore()


def test_tier_switch_through_the_gated_path(gated):
    """512 markers at b = 3e-7 |vara| with the tight budget (1e-7) in force: all flagged and re-evaluated.  513: the default budget is
    enforced and none of them is flagged."""
    sc, v64 = gated
    torch, hdr = sc.torch, sc.hdr
    assert (hdr["budget"], hdr["budget_loose"]) == (ct.TIGHT, ct.LOOSE)
    for m in (ct.CERT_TIGHT_MAX, ct.CERT_TIGHT_MAX + 1):
        sc.restore()
        _, v0 = sc.host()
        b0 = sc.bounds()
        assert ct.over_tight(v0, b0, hdr["budget"]) == 0
        rows = ct.spread(LM, m + 1, seed=m)
        peak, rows = rows[m // 2], np.delete(rows, m // 2)
        v1 = v0.copy()
        v1[rows] = b0[rows] / 3e-7
        sc.put(vara=v1)
        b1 = sc.bounds()                                                  # vara enters the bound through 2^-48 |vara - diag| alone
        assert np.all(np.abs(b1[rows] / v1[rows] / 3e-7 - 1.0) < 1e-3)
        _away_from_the_flag_edges(v1, b1, hdr)
        a1 = sc.plant(np.array([peak]), v1, b1)
        sc.put(a=a1)
        tight = ct.over_tight(v1, b1, hdr["budget"], a1)
        want = ct.select(a1, v1, b1, ct.lower_bound(a1, v1, b1), hdr["budget"], hdr["budget_loose"], tight)
        assert tight == m and want.flagged == (m if m <= ct.CERT_TIGHT_MAX else 0) and want.count == want.flagged + 1
        planted = sc.sh.vara[:LM].clone()
        info, idx = _certify(sc)
        print("gated path, %d over the tight threshold: restatement flagged %d count %d | device %r" % (m, want.flagged, want.count, info))
        assert (info["over_tight"], info["flagged"], info["reevaluated"], info["overflow"]) == (m, want.flagged, want.count, 0)
        assert np.array_equal(idx, want.idx)
        got = sc.sh.vara[:LM]
        sel = torch.from_numpy(want.idx).to(sc.sh.dev)
        mask = torch.zeros(LM, dtype=torch.bool, device=sc.sh.dev)
        mask[sel] = True
        assert torch.equal(got[mask], v64[mask]) and torch.equal(got[~mask], planted[~mask])
    sc.restore()
