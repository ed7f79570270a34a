"""The case tables and exactness premises of tests/test_gpu_fwd_dgrad.py, checked on a machine without a GPU.

For every (case, mode) of the GPU file: the library's host-side row functions and the restated pickers against the table's literal form and
row count; the exact-class and sparse operands with their mass conditions in float64; no masked pre-activation at 0; and the exact checker
reports a reference with ONE product removed as a difference of at least q."""
import pytest
import torch

import test_gpu_fwd_dgrad as T

CASES = T.all_cases()
IDS = [f"s{sec}-{mode}-" + "x".join(map(str, case)) for sec, case, mode, form, rows, seam in CASES]


@pytest.fixture(scope="module")
def cd():
    from artiboost_amd import _lib
    return _lib.cdll()


def test_tables_cover_what_the_issue_lists():
    forms = {form for _, _, _, form, _, _ in CASES}
    for g in range(1, 9):
        for tmpl in (f"c3<{g},FLIP=0,X3=1>", f"c3<{g},FLIP=1,X3=1>", f"c3<{g},FLIP=1,X3=2>"):
            assert tmpl in forms, tmpl
    for tmpl in ("c3r<0>", "c3r<1>", "c3r<1,1,addend,mask>", "cp<256,64,false,0>", "cp<128,64,true,0>", "cp<256,64,false,1>", "cp<128,64,true,1>",
                 "cp<256,64,false,1>+bn", "cp<128,64,true,1>+bn", "c22<256,64,4,false>", "c22<128,64,4,true>", "c22<256,128,1,false>",
                 "c22<256,64,1,false>", "c22<256,64,1,true>", "g2x<64,64,2>", "g2x<64,64,3>", "g2x<64,128,2>", "g2x<64,128,3>", "g2x<128,64,2>",
                 "g2x<128,64,3>", "g2x<128,128,2>", "g2x<64,64,2,nclass=4>", "g2x<64,64,2,nclass=4,ALT>", "g2x<64,64,3,nclass=4,ALT>",
                 "g2x<64,128,2,nclass=4,ALT>", "g2x<64,128,3,nclass=4,ALT>", "g2x<64,128,3,nclass=4>", "g2x<128,64,2,nclass=4>",
                 "g2x<128,64,2,nclass=4,ALT>", "g2x<128,64,3,nclass=4,ALT>", "g2x<128,128,2,nclass=4,ALT>", "g2x<128,128,2,nclass=4>",
                 "g2x<64,64,2>+bn", "g2x<64,128,2>+bn", "g2x<64,128,3>+bn", "gemm_rw<1>", "gemm_rw<2>", "gemm_rw<3>", "gemm_rw<4>"):
        assert tmpl in forms, tmpl
    assert len(set((case, mode) for _, case, mode, _, _, _ in CASES)) == len(CASES), "a (case, mode) pair appears twice"
    assert {c[3] // 64 for c, _, _ in T.SAM} == {1, 2, 3, 4}, "gemm_rw<K / 64, SAM> for every K"
    table = {(case, mode) for _, case, mode, _, _, _ in CASES}
    for prm in T.GUARD:          # the guarded launches are table entries: their route and conditions are checked below
        assert tuple(prm.values) in table, prm.values
    for case, C, D in T.SAM:
        assert (case, "fwd") in table or (case, "fwd_bias") in table
        T.assert_conditions(T.problem(case, "fwd_bias", T.exact_class(case, "fwd_bias")), "fwd_bias")


@pytest.mark.parametrize("sec,case,mode,form,rows,seam", CASES, ids=IDS)
def test_route_table_against_the_library_and_the_restated_pickers(cd, sec, case, mode, form, rows, seam):
    assert T.route(case, mode) == (form, rows)
    assert T.library_rows(cd, case, mode) == rows
    N, H, W, Cin, Cout, k, s, p = case
    if (k, s, p) == (1, 1, 0) and mode in ("fwd", "fwd_bias") and (H * W) % 64 == 0 and Cout % 32 == 0:
        # gemm_rw_ok, as ab_conv1x1_sam_fwd_x3_ok exposes it: the one host-side witness of gemm_rw against the generic kernel
        assert bool(cd.ab_conv1x1_sam_fwd_x3_ok(N, H, W, Cin, Cout // 32, 32)) == form.startswith("gemm_rw"), (case, form)
    if form.startswith("gemm_rw"):
        assert (N * H * W) % 64 == 0 and Cin in (64, 128, 192, 256)


def test_conv3x3r_limit_and_the_fused_epilogue_shortcut(cd):
    """What separates neighbours in the table: 63 against 64 tiles of 8 x 16, and the W >= 24 shortcut that the fused epilogue does not take."""
    assert cd.ab_conv2d_x3_stat_rows(1, 56, 144, 64, 64, 3, 3, 1, 1) == 63 and cd.ab_conv2d_dgrad_x3_bn_rows(1, 56, 144, 64, 64, 3, 3, 1, 1) == 70
    assert cd.ab_conv2d_x3_stat_rows(1, 64, 128, 64, 64, 3, 3, 1, 1) == 64 and cd.ab_conv2d_dgrad_x3_bn_rows(1, 64, 128, 64, 64, 3, 3, 1, 1) == 64
    assert cd.ab_conv2d_x3_stat_rows(5, 64, 112, 64, 64, 3, 3, 1, 1) == 256
    # (1, 8, 32, 64, 64) of the table has 2 tiles either way; at (1, 8, 48) geometry 4 has 3 tiles of 8 x 16 and the fused epilogue's
    # geometry 1 has 2 x 2 = 4 of 4 x 32 -- the counts differ
    assert cd.ab_conv2d_x3_stat_rows(1, 8, 48, 64, 64, 3, 3, 1, 1) == 3 and cd.ab_conv2d_dgrad_x3_bn_rows(1, 8, 48, 64, 64, 3, 3, 1, 1) == 4
    assert T.c3_route(1, 8, 48, 64, 64, True) == (4, 3) and T.c3_route(1, 8, 48, 64, 64, False) == (1, 4)


def _classes(mode, case):
    cls = [T.exact_class(case, mode)]
    if "stats" in mode or "bn_" in mode:
        cls.append("sparse")
    return cls


@pytest.mark.parametrize("sec,case,mode,form,rows,seam", CASES, ids=IDS)
def test_exactness_conditions_and_checker_sensitivity(sec, case, mode, form, rows, seam):
    for cls in _classes(mode, case):
        o = T.problem(case, mode, cls)
        T.assert_conditions(o, mode)
        # planes: hi is exact in bf16, lo is exact in bf16, hi + lo is exact in fp32
        for t in (o.a, o.w) + ((o.a2, o.w2) if o.a2 is not None else ()):
            assert torch.equal(t.hi.bfloat16().float(), t.hi) and torch.equal(t.lo.bfloat16().float(), t.lo)
            assert torch.equal(t.full.double(), t.hi.double() + t.lo.double())
            assert torch.equal((t.full - t.full.bfloat16().float()).bfloat16().float(), t.lo) and torch.equal(t.full.bfloat16().float(), t.hi)
        # every reference value is a multiple of q
        assert bool(((o.ref / o.q) == (o.ref / o.q).round()).all())
        # one product removed from one output element: at least q, and the checker says so
        ref = o.ref_add if mode.endswith("_add") else o.ref
        wrong = ref.clone()
        idx = tuple(int(v) // 2 for v in ref.shape)
        if not ("relu" in mode and float(ref[idx]) == 0.0):          # (a clamped element hides its pre-activation)
            wrong[idx] -= _one_product(o, case, idx)
            if "relu" in mode:
                wrong[idx] = max(float(wrong[idx]), 0.0)
        if float(wrong[idx]) != float(ref[idx]):
            assert abs(float(wrong[idx]) - float(ref[idx])) >= o.q
            with pytest.raises(AssertionError, match=r"1 of \d+ entries differ"):
                T.assert_exact("one product removed", wrong.float(), ref, o.q)
        T.assert_exact("the reference itself", ref.float(), ref, o.q)
        if "bn_" in mode:
            dz, s0, s1, m0, m1 = T.bn_results(o, False)
            assert float(o.pre.abs().min()) >= 0.5
            assert bool(((o.xhat * 2) == (o.xhat * 2).round()).all()) and float(o.xhat.abs().max()) <= 8.0
            assert cls != "sparse" or bool((s1 * 2 == (s1 * 2).round()).all())
            frac = float(o.mask.mean())
            assert 0.2 <= frac <= 0.8, f"the mask keeps {frac:.2f} of the elements: too one-sided to test it"
        if cls == "sparse":
            nz = float((o.ref != 0).double().mean())
            reach = 0.25 if (not o.fwd and case[5:7] == (1, 2)) else 1.0      # a 1x1 / s2 data gradient reaches one input pixel in four
            assert nz >= 0.25 * reach, f"the sparse draw leaves only {nz:.2f} of the outputs non-zero"


def _one_product(o, case, idx):
    """A non-zero hi * hi product that contributes to output element idx (0.0 when the draw has none there)."""
    N, H, W, Cin, Cout, k, s, p = case
    n, y, x, c = idx
    if o.fwd:
        for i in range(k):
            for j in range(k):
                yy, xx = y * s - p + i, x * s - p + j
                if 0 <= yy < H and 0 <= xx < W:
                    for ci in range(Cin):
                        v = float(o.a.hi[n, yy, xx, ci]) * float(o.w.hi[c, i, j, ci])
                        if v:
                            return v
        return 0.0
    Ho, Wo = T._geom(case)
    for i in range(k):
        for j in range(k):
            if (y + p - i) % s or (x + p - j) % s:
                continue
            yy, xx = (y + p - i) // s, (x + p - j) // s
            if 0 <= yy < Ho and 0 <= xx < Wo:
                for co in range(Cout):
                    v = float(o.a.hi[n, yy, xx, co]) * float(o.w.hi[co, i, j, c])
                    if v:
                        return v
    return 0.0


def test_the_kept_plane_products_are_what_the_reference_sums():
    """op(a, w_hi) + op(a_hi, w_lo) == hi*hi + hi*lo + lo*hi, written out, on one small case of each direction."""
    for case, mode in (((1, 9, 7, 64, 40, 3, 1, 0), "fwd_stats"), ((3, 14, 10, 64, 128, 3, 2, 1), "dgrad")):
        o = T.problem(case, mode, "split")
        f = lambda a, w: T._op(case, o.fwd, a, w)
        assert torch.equal(o.ref, f(o.a.hi, o.w.hi) + f(o.a.hi, o.w.lo) + f(o.a.lo, o.w.hi))
        assert not torch.equal(o.ref, f(o.a.full, o.w.full)), "the lo * lo product is invisible in this draw"
