"""The case tables, exactness premises, checkers and bound functions of tests/test_gpu_bn_pool.py, checked on a machine without a GPU.

The tables against the forms the issue lists and against the library's own host-side predicates (ab_col_stats_nparts,
ab_bn_fin_apply_x3_ok, ab_bn_relu_maxpool_bwd_x3_nparts); the exact-class premises in float64 for every case; the checkers against four
planted errors (one row dropped from a statistic, the LAST maximum as the pool winner, running statistics updated twice, dy without its
xhat * k2 term); and the random-class bound functions against a float32 emulation of the kernels' summation order."""
import ctypes

import pytest
import torch

import test_gpu_bn_pool as T

CASES = T.all_cases()
F32, BF16 = T.F32, T.BF16


@pytest.fixture(scope="module")
def cd():
    from artiboost_amd import _lib
    return _lib.cdll()


def _forms(section=None):
    return {form for sec, _, _, _, form in CASES if section in (None, sec)}


def _has(section, *needles):
    return any(all(n in form for n in needles) for form in _forms(section))


# ---------------------------------------------------------------- table coverage
def test_tables_cover_what_the_issue_lists():
    assert len(set((sec, entry, dt, shape) for sec, entry, dt, shape, _ in CASES)) == len(CASES), "a case appears twice"
    # 1. statistics: channel-vector counts that do not divide 256, the narrow and wide edges, both red_rows, the one-row last block
    for needles in (("col_stats<f32>", "vc=24 rl=10"), ("col_stats<bf16>", "vc=5 rl=51"), ("col_stats<f32>", "vc=1 "), ("col_stats<bf16>", "vc=1 "),
                    ("col_stats<f32>", "vc=256"), ("col_stats<bf16>", "vc=256"), ("col_stats<f32>", "red_rows=32"), ("col_stats<bf16>", "red_rows=32"),
                    ("col_stats<f32>", "last=1"), ("col_stats<bf16>", "last=1"), ("col_stats_x3", "vc=5 rl=51"), ("col_stats_x3", "vc=256"),
                    ("colsum_finalize", "rows=1"), ("colsum_finalize", "rows=513")):
        assert _has(1, *needles), needles
    shapes1 = {(dt, shape) for sec, entry, dt, shape, _ in CASES if sec == 1 and entry == "ab_col_stats"}
    for dt, Cs in ((F32, (4, 8, 64, 96, 1024)), (BF16, (8, 40, 64, 96, 1024, 2048))):
        for C in Cs:
            for M in (1, 15, 16, 17, 33, 1000):
                assert (dt, (M, C)) in shapes1, (dt, M, C)
        assert any(s[0] == 16400 for d, s in shapes1 if d == dt)
    # 2. the three loops of reduce_parts_1024, with and without the c < C guard, forward and backward finalize
    for k in ("bn_finalize<8>", "bn_bwd_finalize<8>"):
        for loop in ("tail", "2-deep", "8-deep"):
            assert _has(2, k, loop) and _has(2, k, loop, "c<C"), (k, loop)
    rows2 = {shape for sec, entry, dt, shape, _ in CASES if sec == 2}
    assert rows2 == {(r, C) for r in (1, 7, 128, 129, 300, 897, 1100) for C in (4, 12, 64, 100)}
    # 3. generic apply / backward, fixed and per-iteration, both dtypes, the sliced reduction, one wrap per path
    for dt in (F32, BF16):
        for fx in ("fixed", "per-iteration"):
            assert _has(3, f"bn_apply<{dt}>", fx) and _has(3, f"bn_bwd_apply<{dt}>", fx), (dt, fx)
        for vc in (2 if dt == F32 else 1, 24 if dt == F32 else 12):
            assert _has(3, f"bn_bwd_reduce<{dt}> vc={vc} "), (dt, vc)
    assert _has(3, "ysl=2") and _has(3, "bn_apply<f32> fixed wrap") and _has(3, "bn_apply<f32> per-iteration wrap")
    assert _has(3, "bn_bwd_apply<f32> fixed wrap") and _has(3, "bn_bwd_apply<f32> per-iteration wrap")
    shapes3 = {(dt, shape) for sec, entry, dt, shape, _ in CASES if sec == 3}
    for dt in (F32, BF16):
        for C in (8, 24, 96, 64, 512):
            for M in (2, 64, 1024, 1000):
                assert (dt, (M, C)) in shapes3
    # 4. the split-plane producers
    for k in ("bn_apply_x3<false>", "bn_apply_x3<true>", "bn_apply_x3<false,true>"):
        for fx in ("fixed", "per-iteration", "fixed wrap", "per-iteration wrap"):
            assert _has(4, k + " " + fx), (k, fx)
    for r in ("none", "f32", "planes"):
        assert _has(4, "bn_apply_x3_c4 res=" + r)
    assert {shape[1] for sec, e, dt, shape, form in CASES if "bn_apply_x3_c4" in form} == {4, 12, 36}
    assert {shape[1] for sec, e, dt, shape, form in CASES if sec == 4 and e == "ab_bn_apply_x3" and "c4" not in form and "wrap" not in form} == {8, 96, 64, 2048}
    fin = {shape for sec, e, dt, shape, _ in CASES if e == "ab_bn_fin_apply_x3"}
    assert {(r, M, 64) for r in (1, 3, 4, 5, 64) for M in (1, 31, 33, 1056)} <= fin and (5, 40000, 64) in fin and (5, 1100, 2048) in fin
    assert _has(4, "bn_fin_apply_x3", "strip wrap") and _has(4, "bn_fin_apply_x3", "nsl=32")
    for mk in T.MASKS:
        assert _has(4, "bn_fin_bwd_apply_x3 mask=" + mk) and _has(4, "bn_bwd_finalize<8>+bn_bwd_apply_x3 mask=" + mk)
        assert _has(4, "bn_fin_bwd_apply_x3 mask=" + mk, "given") and _has(4, "bn_bwd_apply_x3 mask=" + mk, "given")
        assert _has(4, "bn_fin_bwd_apply_x3 mask=" + mk, "ysl=2") and _has(4, "bn_bwd_apply_x3 mask=" + mk, "ysl=2")
    assert _has(4, "bn_bwd_apply_x3 fixed wrap") and _has(4, "bn_bwd_apply_x3 per-iteration wrap")
    # 5. the stem pool: every kernel, every geometry the issue names
    for k in ("maxpool_fwd<f32>", "maxpool_fwd<bf16>", "maxpool_bwd<f32>", "maxpool_bwd<bf16>", "bn_bwd<f32>+pool_idx", "bn_bwd<bf16>+pool_idx",
              "maxpool_fwd<f32>+planes", "maxpool_fwd_x3", "maxpool_fwd_x3+ywin", "maxpool_fwd_x3+ywin,out=NULL", "pool_win_bn_reduce+pool_bwd_bn_apply_x3",
              "pool_bwd_bn_reduce<8,false>+pool_bwd_bn_apply_x3", "nparts=0: maxpool_bwd+bn_bwd_x3(recompute)"):
        assert _has(5, k), k
    for geo in ("W=2", "H=2", "Ho<PFX_ROWS", "Ho%PFX_ROWS", "C/4=256"):
        assert _has(5, "maxpool_fwd_x3", geo), geo
    assert {shape[:4] for sec, e, dt, shape, _ in CASES if sec == 5} == {(1, 2, 2, 8), (2, 4, 2, 8), (1, 6, 10, 64), (2, 10, 6, 64), (1, 16, 16, 64),
                                                                        (3, 8, 12, 96), (1, 8, 8, 12), (1, 4, 4, 1024)}
    # 6. the average pool
    assert _has(6, "avgpool_fwd<f32>", "HW=1") and _has(6, "avgpool_fwd<f32>", "ragged") and _has(6, "avgpool_fwd<bf16>")
    assert {shape for sec, e, dt, shape, _ in CASES if sec == 6 and dt == F32} == {(1, 1, 4), (3, 49, 132), (2, 7, 512), (64, 16, 2048)}


# ---------------------------------------------------------------- the library's predicates against the restated ones
def test_row_counts_and_predicates_against_the_library(cd):
    Ms = {1, 15, 16, 17, 33, 1000, 1024, 1040, 16400, 16384, 16385, 40000, 87383, 174764, 8194, 1 << 20, (1 << 20) + 1, 3 << 20}
    for sec, entry, dt, shape, form in CASES:
        if sec in (1, 3) or (sec == 4 and len(shape) == 2):
            Ms.add(shape[0])
    for M in sorted(Ms):
        assert cd.ab_col_stats_nparts(ctypes.c_long(M)) == T.nparts(M), M
        assert T.red_rows(M) % 16 == 0 and T.red_rows(M) >= 16 and (T.nparts(M) - 1) * T.red_rows(M) < M <= T.nparts(M) * T.red_rows(M)
    assert T.red_rows(16384) == 16 and T.red_rows(16400) == 32 and T.nparts(33) == 3 and T.nparts(16400) == 513
    for rows in (0, 1, 3, 4, 5, 63, 64, 65, 70, 128):
        for C in (4, 12, 64, 96, 128, 1024, 2048):
            assert bool(cd.ab_bn_fin_apply_x3_ok(rows, C)) == T.bnfin_ok(rows, C), (rows, C)
    for N, H, W, C in T.POOL + ((2, 64, 64, 64), (1, 3, 4, 8), (1, 4, 3, 8), (1, 4, 4, 2048), (1, 8, 8, 40)):
        assert cd.ab_bn_relu_maxpool_bwd_x3_nparts(N, H, W, C) == T.pool_rows(N, H, W, C), (N, H, W, C)
    assert T.pool_rows(3, 8, 12, 96) == 0 and T.pool_rows(1, 8, 8, 12) == 0 and T.pool_rows(2, 10, 6, 64) == 2 and T.pool_rows(1, 4, 4, 1024) == 4
    for M, C, given, route in T.BWDX3:
        assert (route == "fin") == T.bnfin_ok(given or T.nparts(M), C), (M, C, given)
        assert (route == "fin") == bool(cd.ab_bn_fin_apply_x3_ok(given or cd.ab_col_stats_nparts(ctypes.c_long(M)), C))
    # the wrap cases are the smallest M past 8192 x 256 vectors, plus one row
    for dt, M, C in T.WRAP_GEN:
        assert T.wraps((M - 1) * C // T.VEC[dt]) and not T.wraps((M - 2) * C // T.VEC[dt])
    for M, C in T.WRAP_X3:
        assert T.wraps((M - 1) * C // 8) and not T.wraps((M - 2) * C // 8) and not T.bnfin_ok(T.nparts(M), C)
    assert T.bnfin_grid(40000, 64) == 1024 < T.cdiv(40000, 32) and T.bnfin_grid(1100, 2048) == 32 * 32 and T.bnfin_grid(1, 64) == 1
    assert [T.fixed(4, C) for C in T.GEN_C] == [True, False, False, True, True] and [T.fixed(8, C) for C in T.X3_C] == [True, False, True, True]
    assert [T.rp_loops(r) for r in T.FIN_ROWS] == ["tail", "tail", "tail", "2-deep", "2-deep", "8-deep", "8-deep"]


# ---------------------------------------------------------------- premises of the exact class
def _planes_exact(v):
    """hi + lo == v for the bf16 pair split() returns."""
    f = v.float()
    hi = f.bfloat16().float()
    lo = (f - hi).bfloat16().float()
    return torch.equal(hi.double() + lo.double(), v)


BN_SHAPES = sorted({(shape[0], shape[1]) for sec, e, dt, shape, _ in CASES if sec == 3 and shape[0] <= 4096} |
                   {(M, C) for M, C, _, _ in T.BWDX3} | {(66, C) for C in T.X3_C + T.C4_C} | {(33, 96)})


@pytest.mark.parametrize("M,C", BN_SHAPES, ids=lambda v: str(v))
def test_exact_class_premises_batchnorm(M, C):
    for seed, balanced in ((0, M % 2 == 0), (8, M % 2 == 0), (4, False)):
        o = T.exact_problem(M, C, seed, balanced=balanced)
        T.assert_sum_conditions(o.y)
        if balanced:
            assert bool((o.s.sum(0) == 0).all()), "signs are not balanced"
            bnp, var = T.ref_bnp(o.y, o.gamma, o.beta, 0.0)
            assert torch.equal(bnp, o.bnp) and torch.equal(var, o.sigma ** 2), "mean / var / invstd are not the hand-built ones"
        xhat = (o.y - o.bnp[2]) * o.bnp[3]
        assert torch.equal(xhat, o.s), "xhat is not +-1"
        for res, rb in ((None, None), (o.res, None), (o.res_y, o.bnp2)):
            pre = T.ref_apply(o.y, o.bnp, False, res, rb)
            assert bool(((pre * 2) % 2 == 1).all()) and float(pre.abs().min()) >= 0.5, "a pre-activation is not an odd multiple of 1/2"
            out = pre.clamp_min(0)
            assert torch.equal(out.float().double(), out) and torch.equal(out.bfloat16().double(), out) and _planes_exact(out)
        dz, db, dg, dy = T.ref_bwd(o.dout, o.y, o.bnp, (T.ref_apply(o.y, o.bnp, True, o.res) > 0).double())
        assert bool((db == db.round()).all()) and bool((dg == dg.round()).all()) and float(db.abs().max()) <= T.LIM
        if (M & (M - 1)) == 0:
            assert torch.equal(dy.float().double(), dy), "dy is not representable in fp32 at a power-of-two M"
        for t in (o.y, o.res, o.dout, o.res_y, o.bnp, o.bnp2):
            assert torch.equal(t.bfloat16().double(), t), "an operand is not representable in bf16"


@pytest.mark.parametrize("dt,M,C", T.stats_cases(), ids=lambda v: str(v))
def test_exact_class_premises_statistics(dt, M, C):
    o = T.exact_problem(M, C, 1, balanced=False)
    T.assert_sum_conditions(o.y)
    assert torch.equal(o.y.to(T.TD[dt]).double(), o.y)
    ref = T._block_sums(o.y, M)
    assert ref.shape == (T.nparts(M), C, 2) and torch.equal(ref.sum(0)[:, 0], o.y.sum(0)) and torch.equal(ref.float().double(), ref)
    vc, rl = T.lanes(dt, C)
    assert 1 <= vc <= 256 and rl == 256 // vc and f"vc={vc} rl={rl} red_rows={T.red_rows(M)}" in T.stats_form(dt, M, C)
    # planted error: one row dropped from one block's statistic
    if M > 1:
        wrong = ref.clone()
        wrong[-1, :, 0] -= o.y[M - 1]
        wrong[-1, :, 1] -= o.y[M - 1] ** 2
        with pytest.raises(AssertionError, match="entries differ"):
            T.assert_bits("one row dropped", wrong.float(), ref)
    T.assert_bits("the reference itself", ref.float(), ref)


@pytest.mark.parametrize("rows", T.FIN_ROWS + T.FINAPP_ROWS)
@pytest.mark.parametrize("C", (4, 12, 64, 100))
def test_hand_built_rows_give_the_hand_built_batchnorm(rows, C):
    for count in (4 * rows, 64):
        p = T._fin_problem(rows, C, count, 1)
        assert bool((p.part == p.part.round()).all()) and float(p.part.abs().max()) < 2 ** 24
        S, Q = p.part[:, :, 0].sum(0), p.part[:, :, 1].sum(0)
        mean = S / count
        var = Q / count - mean * mean
        assert torch.equal(mean, p.mu) and torch.equal(var, p.sigma ** 2)
        assert torch.equal(T.hand_bnp(mean, torch.sqrt(var), p.gamma, p.beta), p.bnp) and torch.equal(p.bnp.float().double(), p.bnp)
        for m in (0.5, 0.25):
            rm, rv = T.ref_running(p.rm0, p.rv0, mean, var, count, m)
            assert torch.equal(rm.float().double(), rm), "running_mean is not exact"


@pytest.mark.parametrize("shape", T.POOL, ids=lambda v: "x".join(map(str, v)))
def test_exact_class_premises_pool(shape):
    N, H, W, C = shape
    o = T.pool_problem(shape)          # (ref_pool asserts inside that torch's winner is the first maximum)
    assert float(o.pre.abs().min()) >= 0.5 and bool(((o.pre * 2) % 2 == 1).all())
    assert _planes_exact(o.pooled) and torch.equal(o.pooled.bfloat16().double(), o.pooled)
    # the draw ties: some window holds its maximum more than once, and not only at 0
    _, last_code, _ = T.scan_pool(o.act, last=True)
    tied = (last_code != o.code)
    assert bool(tied.any()), "no window ties"
    assert bool((o.pooled[tied] > 0).any()), "only post-ReLU zeros tie"
    assert int(o.code.min()) >= 0 and int(o.code.max()) <= 8
    if H >= 4 and W >= 4:
        assert len(o.code.unique()) >= 5
    assert torch.equal(T.pool_gather(o.act, o.flat), o.pooled) and torch.equal((T.pool_gather(o.y4, o.flat) * o.bnp[0] + o.bnp[1]).clamp_min(0), o.pooled)
    assert torch.equal(o.da.sum((0, 1, 2)), o.dpool.sum((0, 1, 2)))
    assert bool((o.db == o.db.round()).all()) and bool((o.dg == o.dg.round()).all())
    # the reduction over the pooled elements (x3w) is the same sum: linearity
    mw = ((o.ywin * o.bnp[0] + o.bnp[1]) > 0).double()
    xw = (o.ywin - o.bnp[2]) * o.bnp[3]
    assert torch.equal((o.dpool * mw).sum((0, 1, 2)), o.db) and torch.equal((o.dpool * mw * xw).sum((0, 1, 2)), o.dg)
    # planted error: the LAST maximum as the winner
    with pytest.raises(AssertionError, match="entries differ"):
        T.assert_bits("last maximum", last_code.to(torch.uint8), o.code.double())
    T.assert_bits("first maximum", o.code.to(torch.uint8), o.code.double())


# ---------------------------------------------------------------- checker sensitivity
def test_checkers_fail_on_the_planted_errors():
    p = T._fin_problem(7, 12, 28, 1)
    mean, var = p.mu, p.sigma ** 2
    for m in (0.5, 0.25):
        rm1, rv1 = T.ref_running(p.rm0, p.rv0, mean, var, p.count, m)
        T.assert_running_once("one update", rm1.float(), rv1.float(), p.rm0, p.rv0, mean, var, p.count, m)
        rm2, rv2 = T.ref_running(rm1, rv1, mean, var, p.count, m)          # updated twice
        assert not torch.equal(rm2, rm1)
        with pytest.raises(AssertionError):
            T.assert_running_once("two updates", rm2.float(), rv2.float(), p.rm0, p.rv0, mean, var, p.count, m)
        # running_var alone updated twice
        if not torch.equal(rv2.float(), rv1.float()):
            with pytest.raises(AssertionError, match="ulp"):
                T.assert_running_once("two updates of the variance", rm1.float(), rv2.float(), p.rm0, p.rv0, mean, var, p.count, m)
    for M in (64, 1000):
        o = T.exact_problem(M, 24, 0)
        mask = (T.ref_apply(o.y, o.bnp, True) > 0).double()
        dz, db, dg, dy = T.ref_bwd(o.dout, o.y, o.bnp, mask)
        _, _, _, wrong = T.ref_bwd(o.dout, o.y, o.bnp, mask, keep_k2=False)
        assert bool((dg != 0).any())
        if M == 64:
            with pytest.raises(AssertionError, match="entries differ"):
                T.assert_bits("dy without xhat * k2", wrong.float(), dy)
            T.assert_bits("dy", dy.float(), dy)
        else:
            _, _, e_dy = T.bwd_bound(o.dout, o.y, o.bnp, mask, 10, 16, exact_sums=True)
            with pytest.raises(AssertionError, match="first-order bound"):
                T.assert_bound("dy without xhat * k2", wrong.float(), dy, e_dy)
            T.assert_bound("dy", dy.float(), dy, e_dy)
    # a zero bound demands equality
    with pytest.raises(AssertionError):
        T.assert_bound("zero bound", torch.tensor([1e-30]), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))


# ---------------------------------------------------------------- the bound functions on a float32 emulation of the summation order
def emu_col_sums(cols, rl, rows):
    """Column sums of each float32 [M, C] in `cols` as the reduction kernels form them: per workgroup of `rows` rows, lane rr adds rows
    rr, rr + rl, ... in order, then the rl lane sums are added in order (both in float32); the workgroup rows are then added in double."""
    M = cols[0].shape[0]
    tot = [torch.zeros(c.shape[1], dtype=torch.float64) for c in cols]
    for r0 in range(0, M, rows):
        for k, c in enumerate(cols):
            blk = c[r0:r0 + rows]
            n = T.cdiv(blk.shape[0], rl)
            pad = torch.zeros((n * rl, c.shape[1]), dtype=torch.float32)
            pad[:blk.shape[0]] = blk
            pad = pad.view(n, rl, -1)
            lane = torch.zeros((rl, c.shape[1]), dtype=torch.float32)
            for i in range(n):
                lane = lane + pad[i]
            a = torch.zeros(c.shape[1], dtype=torch.float32)
            for j in range(rl):
                a = a + lane[j]
            tot[k] += a.double()
    return tot


@pytest.mark.parametrize("M,C,ratio", ((1000, 96, 2), (4096, 64, 0), (4096, 64, 8), (4096, 64, 64), (4099, 8, 2), (600, 1024, 2)))
def test_bounds_hold_on_a_float32_emulation(M, C, ratio):
    o = T._random_problem(M, C, ratio, 0)
    vc, rl = T.lanes(F32, C)
    rows, eps = T.red_rows(M), 1e-5
    y = o.y.float()
    S, Q = emu_col_sums([y, y * y], rl, rows)
    eS, eQ = T.stats_bound(o.y, rl)
    w = f"emulation {(M, C, ratio)}"
    T.assert_bound(w + " sum x", S, o.y.sum(0), eS)
    T.assert_bound(w + " sum x^2", Q, (o.y * o.y).sum(0), eQ)
    # bn_finalize_kernel: double up to invstd, then float32
    mean = S / M
    var = (Q / M - mean * mean).clamp_min(0)
    invstd = (1.0 / torch.sqrt(var + eps)).float()
    sc = o.gamma.float() * invstd
    sh = o.beta.float() - mean.float() * sc
    got = torch.stack([sc, sh, mean.float(), invstd])
    ref, _ = T.ref_bnp(o.y, o.gamma, o.beta, eps)
    e_bnp = T.bnp_bound(o.y, o.gamma, o.beta, eps, eS, eQ)
    for k, name in enumerate(("scale", "shift", "mean", "invstd")):
        T.assert_bound(f"{w} {name}", got[k], ref[k], e_bnp[k])
    out = torch.relu(y * sc + sh + o.res.float())
    T.assert_bound(w + " out", out, T.ref_apply(o.y, ref, True, o.res), T.apply_bound(o.y, ref, e_bnp, o.res))
    # backward on the emulated float32 bnp, the reference reading the same values
    b64 = got.double()
    pre = o.y * b64[0] + b64[1]
    mask32 = (y * sc + sh > 0)
    dz32 = torch.where(mask32, o.dout.float(), torch.zeros_like(y))
    xhat32 = (y - got[2]) * got[3]
    s0, s1 = emu_col_sums([dz32, dz32 * xhat32], rl, rows)
    mask = (pre > 0).double()
    dz, db, dg, dy = T.ref_bwd(o.dout, o.y, b64, mask)
    e_db, e_dg, e_dy = T.bwd_bound(o.dout, o.y, b64, mask, rl, rows, pre=pre)
    T.assert_bound(w + " dbeta", s0, db, e_db)
    T.assert_bound(w + " dgamma", s1, dg, e_dg)
    invM = torch.tensor(1.0 / M, dtype=torch.float32)
    k1, k2 = s0.float() * invM, s1.float() * invM
    dy32 = sc * (dz32 - k1 - xhat32 * k2)
    T.assert_bound(w + " dy", dy32, dy, e_dy)
    # the bound is a bound, not a blanket: at four times the margin it still separates a variance computed from one row fewer
    wrong, _ = T.ref_bnp(o.y[1:], o.gamma, o.beta, eps)
    if ratio <= 8:
        with pytest.raises(AssertionError, match="first-order bound"):
            T.assert_bound(w + " invstd of M - 1 rows", wrong[3].float(), ref[3], e_bnp[3])
