"""The case tables, operands and float64 reference of tests/test_gpu_head_forms.py, checked on a machine without a GPU.

The tables against the codes ab_softargmax3d_form (host only) can return and against the edges the file is there for; every case's
expected form against the witness; the float64 reference against learner_oracle.softargmax3d in fp32 at test_gpu_head.py's tolerances;
the premises of the small-weight-sum cases and of the confidence-gradient cases."""
import pytest
import torch

import learner_oracle as lo
import test_gpu_head_forms as T

CASES = T.all_cases()
F32, BF16 = T.F32, T.BF16
CPU_ELEMS = 400000          # shapes up to this many logits get the fp32 cross-check


@pytest.fixture(scope="module")
def form():
    from artiboost_amd import _lib
    fn = _lib.cdll().ab_softargmax3d_form
    return lambda entry, dt, C, D, DP, norm: fn(entry, T.DTC(dt), C, D, DP, norm)


def _cd(shape):
    return shape[0] * shape[2]


def _pixels(shape):
    return shape[4] * shape[5]


# ---------------------------------------------------------------- the witness against the restated dispatch, everywhere
def test_witness_returns_exactly_the_codes_of_the_tables(form):
    """Every (C, D, DP) with C*DP <= 1024 over a grid of C, D and pitch: the witness equals the restated dispatch, and the codes it returns
    are exactly ALL_FORMS -- each of which is named by at least one table case."""
    seen = {e: set() for e in range(4)}
    for C in (1, 2, 3, 4, 5, 22, 31, 32, 73, 193, 1024):
        for D in range(1, 1024 // C + 1):
            for DP in {D, D + 1, D + 4}:
                if C * DP > 1024:
                    continue
                for e in range(4):
                    if e >= 2 and (C * DP) % 2:
                        assert form(e, F32, C, D, DP, 0) == T.ESHAPE
                        continue
                    for dt in ((F32, BF16) if e < 2 else (F32,)):
                        code = form(e, dt, C, D, DP, (C + D) % 2)
                        assert code == T.restated_form(e, C, D, DP), (e, dt, C, D, DP, code)
                        seen[e].add(code)
    assert {e: tuple(sorted(s)) for e, s in seen.items()} == T.ALL_FORMS
    in_tables = {e: set() for e in range(4)}
    for sec, e, code, dts, shape, variants, what in CASES:
        if sec != 5:
            in_tables[e].add(code)
    assert {e: tuple(sorted(s)) for e, s in in_tables.items()} == T.ALL_FORMS


def test_every_case_names_the_form_the_witness_returns(form):
    assert len(set((sec, e, shape) for sec, e, _, _, shape, _, _ in CASES)) == len(CASES), "a case appears twice"
    for sec, e, code, dts, shape, variants, what in CASES:
        C, D, DP = shape[:3]
        assert f"C*DP={C * DP}" in what or sec == 5, what
        assert ("DP>D" in what) == (DP > D), what
        for dt in dts:
            for v in variants:
                assert form(e, dt, C, D, DP, T.variant(v)[0]) == code, (sec, e, dt, shape, v)


def test_refusal_codes(form):
    for entries, C, D, DP, with_conf, norm, code in T.REFUSALS:
        for e in entries:
            if not with_conf:
                assert form(e, F32, C, D, DP, norm) == code
            else:                    # g_conf is refused by the launcher; the dispatch itself takes the shape
                assert form(e, F32, C, D, DP, norm) == T.restated_form(e, C, D, DP) and norm == 1 and code == T.EINVAL
    assert form(4, F32, 1, 1, 1, 0) == T.EINVAL and form(-1, F32, 1, 1, 1, 0) == T.EINVAL
    from artiboost_amd import _lib
    assert _lib.cdll().ab_softargmax3d_form(0, 2, 1, 1, 1, 0) == T.EINVAL                       # AB_DT_U8N is no logits dtype
    assert form(2, BF16, 1, 2, 2, 0) == T.EINVAL                                                # the split entries read fp32 logits only
    assert form(0, F32, 1, 1, 1, 2) == T.ESHAPE and form(0, F32, 0, 1, 1, 0) == T.ESHAPE and form(0, F32, 1, 0, 1, 0) == T.ESHAPE
    assert form(0, F32, 70000, 70000, 70000, 0) == T.ESHAPE                                     # no overflow of C*DP into range


# ---------------------------------------------------------------- the edges the tables are there for
def test_tables_cover_what_the_file_is_there_for():
    def rows(sec, e=None):
        return [(code, shape, what) for s, en, code, _, shape, _, what in CASES if s == sec and e in (None, en)]
    # stage 1: the listed widths per form, first and last width of every KP, a padded pitch per KP, a D > 32 merge per KP
    want = {10: {1, 15, 33, 45}, 2: {2, 102, 256}, 4: {258, 264, 512}, 6: {514, 616, 704, 768}, 8: {770, 1012, 1024}}
    for key, cds in want.items():
        got = {_cd(shape) for code, shape, _ in rows(1) if (code == 10 if key == 10 else code // 10 == 10 + key)}
        assert cds <= got, (key, cds - got)
        fam = [(code, shape) for code, shape, _ in rows(1) if (code == 10 if key == 10 else code // 10 == 10 + key)]
        assert any(s[2] > s[1] for _, s in fam) and any(s[1] > 32 for _, s in fam), key
        if key != 10:
            assert {c % 10 for c, _ in fam} == {0, 1}, key
    pix = {(s[4], s[5]) for _, s, _ in rows(1)}
    assert {(1, 1), (1, 65), (65, 1), (7, 5), (72, 72), (1, 3)} <= pix and {63, 64, 65} <= {h * w for h, w in pix}
    assert {s[3] for _, s, _ in rows(1)} == {1, 3}
    big = [s for _, s, _ in rows(1) if _pixels(s) == 5184]
    assert sorted(_cd(s) for s in big) == [2, 45, 1024] and all(s[3] == 1 for s in big)
    assert max(s[3] * _pixels(s) * _cd(s) * 4 for _, s, _ in rows(1)) <= 22 * 2 ** 20
    assert sorted(-(-s[4] * s[5] // 64) for s in T.S2) == [1, 2, 81]
    # backward: scalar and pair widths, pixel counts around the 16-pixel workgroup
    assert {_cd(s) for c, s, _ in rows(3) if c == 20} >= {1, 15, 45}
    assert {_cd(s) for c, s, _ in rows(3) if c == 1628} == {2, 50, 616, 1022, 1024}
    assert {_pixels(s) for _, s, _ in rows(3)} >= {1, 15, 16, 17, 63, 64, 65}
    assert any(s[2] > s[1] for _, s, _ in rows(3))
    # split planes: widths per (V, KV), pixel counts, colpart rows through sam_bias_finalize
    for e, base in ((2, 11600), (3, 16400)):
        assert {_cd(s) for c, s, _ in rows(4, e) if c == base + 43} == {4, 704, 768}
        assert {_cd(s) for c, s, _ in rows(4, e) if c == base + 44} == {772, 1024}
        assert {_cd(s) for c, s, _ in rows(4, e) if c == base + 28} == {2, 50, 770, 1022}
    assert {_pixels(s) for _, s, _ in rows(4)} == {1, 15, 16, 17, 63, 64, 65, 5184}
    nrows = {s[3] * -(-_pixels(s) // 64) for _, s, _ in rows(4, 3)}
    assert {1, 3, 32, 33, 81 * 3} <= nrows
    for _, s, what in rows(4, 3):
        assert f"rows={s[3] * -(-_pixels(s) // 64)}" in what
    # small S: both volumes, even and odd widths
    assert {(s[1], s[4], s[5]) for _, s, _ in rows(5)} == {(4, 4, 4), (2, 3, 5)}
    for vol in ((4, 4, 4), (2, 3, 5)):
        assert {_cd(s) % 2 for _, s, _ in rows(5) if (s[1], s[4], s[5]) == vol} == {0, 1}
    assert {e for s, e, *_ in CASES if s == 5} == {0, 1, 2, 3}


# ---------------------------------------------------------------- the reference
def _elems(shape):
    return shape[0] * shape[1] * shape[3] * shape[4] * shape[5]


# every table shape of every section, forward-only ones included (their gradient is cross-checked as well: it costs nothing here)
SMALL = sorted({(dt, shape, T.variant(v), sec == 5) for sec, e, _, dts, shape, vs, _ in CASES for dt in dts for v in vs
                if _elems(shape) <= CPU_ELEMS}, key=str)


def test_only_the_two_large_shapes_stay_out_of_the_fp32_cross_check():
    out = {shape for _, _, _, _, shape, _, _ in CASES if _elems(shape) > CPU_ELEMS}
    assert out == {(32, 32, 32, 1, 72, 72), (5, 9, 10, 3, 72, 72)}


@pytest.mark.parametrize("dt,shape,nv,small_s", SMALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_float64_reference_agrees_with_the_fp32_oracle(dt, shape, nv, small_s):
    """learner_oracle.softargmax3d in fp32 on the same inputs, at test_gpu_head.py::test_head_vs_oracle's tolerances."""
    C, D, DP, B, H, W = shape
    norm, with_conf = nv
    r64 = T.reference(dt, C, D, DP, B, H, W, norm, with_conf, small_s)
    r32 = T.reference(dt, C, D, DP, B, H, W, norm, with_conf, small_s, True, torch.float32)
    assert r64.grad.dtype == torch.float64 and r32.grad.dtype == torch.float32 and r64.grad.shape == (B, C, D, H, W)
    torch.testing.assert_close(r32.uvd.double(), r64.uvd, rtol=0, atol=3e-6)
    torch.testing.assert_close(r32.conf.double(), r64.conf, rtol=3e-5, atol=0.0 if small_s else 1e-8)    # small S: see T.check_forward
    scale = float(r64.grad.abs().max())
    torch.testing.assert_close(r32.grad.double(), r64.grad, rtol=1e-4, atol=1e-5 * scale)


def test_operands_are_what_the_kernel_reads():
    """bf16 operands are bf16 values (the reference upcasts them exactly), the device layout carries PAD_VALUE in the padded slots only."""
    o = T.operands(BF16, 5, 9, 10, 3, 4, 4)
    assert o.core.dtype == torch.bfloat16 and o.g_uvd.dtype == torch.float32
    x = T.nhwc(o.core, 10)
    assert x.shape == (3, 4, 4, 50) and x.dtype == torch.bfloat16
    back = T.from_nhwc(x, 5, 10)
    assert torch.equal(back[:, :, :9], o.core.double()) and bool((back[:, :, 9:] == T.PAD_VALUE).all())
    assert abs(float(T.operands(F32, 22, 28, 28, 3, 9, 7).core.std()) - 3.0) < 0.1


def test_small_s_inputs_are_in_the_regime():
    for C, D, DP, B, H, W, what in T.SMALL_S:
        for dt in (F32, BF16):
            w = T.operands(dt, C, D, DP, B, H, W, True).core.double().sigmoid().reshape(B, C, -1)
            ratio = 1e-7 / w.sum(2)
            assert float(ratio.min()) > 0.05, (what, dt, float(ratio.min()))
            # ... where the softmax constants are off by tens of percent: 1 / (S (1 + 1e-7)) against 1 / (S + 1e-7)
            assert float((1.0 + ratio).min()) > 1.05


def test_confidence_gradient_inputs_have_one_maximum_per_class():
    n = 0
    for sec, e, _, dts, shape, variants, what in CASES:
        if any(T.variant(v)[1] for v in variants):
            for dt in dts:
                C, D, DP, B, H, W = shape
                assert T.unique_max(T.operands(dt, C, D, DP, B, H, W).core), (dt, shape)
                n += 1
    assert n >= 30
    # what the kernels do differently on a tie (the known deviation): torch.max hands the gradient to the first maximal index only
    x = torch.zeros(1, 4, dtype=torch.float64, requires_grad=True)
    torch.max(x, dim=-1).values.sum().backward()
    assert x.grad.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    assert not T.unique_max(torch.zeros(1, 1, 2, 1, 2))
