"""Host side of the device input preparation (``glue.filtfilt``: scipy.signal.filtfilt, infer/modules/vc/pipeline.py:23,221): the
``lfilter_zi`` restatement, the warm-up derived from the poles, the argument checks (scipy's), and what the built library refuses
without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import signal

import prep_cases

FILTERS = [signal.butter(N=5, Wn=48, btype="high", fs=16000), signal.butter(3, 0.2), signal.butter(8, 0.1, "high"), signal.cheby1(4, 1, 0.3),
           signal.butter(2, 0.01), signal.butter(1, 0.5), ([0.5, 0.25], [2.0, -1.0, 0.25]), ([1.0, 2.0, 3.0, 4.0], [1.0, -0.5])]


@pytest.mark.parametrize("k", range(len(FILTERS)))
def test_lfilter_zi_restatement_equals_scipy_bit_for_bit(k):
    from rvc_amd import glue

    b, a = FILTERS[k]
    want = signal.lfilter_zi(b, a)
    got = glue.lfilter_zi(b, a)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


def test_warmup_of_the_pipeline_filter_is_derived_and_within_the_cap():
    """cond(V) rho^W < 2^-64 for the W the wrapper uses, W is the smallest multiple of the lane length that satisfies it, and it lies
    under the cap; a pole radius of 0.9999 is refused, as are an unstable filter and an order above 8."""
    import rvc_amd
    from rvc_amd import glue

    b, a = FILTERS[0]
    W = glue.filt_warmup(a)
    lam, V = np.linalg.eig(np.linalg.inv(np.eye(5)) @ np.vstack([-a[1:], np.eye(5)[:-1]]).T)
    rho, cond = np.abs(lam).max(), np.linalg.cond(V)
    assert 0.9941 < rho < 0.9943 and 1e8 < cond < 1e10
    assert W % glue.FILT_LANE == 0 and 0 < W <= glue.FILT_WARMUP_CAP
    assert np.log(cond) + W * np.log(rho) < -64 * np.log(2) <= np.log(cond) + (W - glue.FILT_LANE) * np.log(rho)
    assert glue.filtfilt_exact_len(b, a) == W + glue.FILT_LANE - 2 * 18
    for bad_a in ([1.0, -1.9998, 0.9998 ** 2], [1.0, -2.5, 1.0]):  # a double pole at 0.9999 (defective, far above the cap); a pole at 2
        with pytest.raises(rvc_amd.RvcmiError):
            glue.filt_warmup(bad_a)
    b9, a9 = signal.butter(9, 0.2)
    with pytest.raises(rvc_amd.RvcmiError):
        glue.filtfilt(torch.zeros(100, dtype=torch.float64), b9, a9)


def test_argument_errors_are_scipys():
    from rvc_amd import glue

    b, a = FILTERS[0]
    for n in (1, 18):  # padlen = 18: scipy refuses n <= padlen
        with pytest.raises(ValueError) as e_ref:
            signal.filtfilt(b, a, np.zeros(n))
        with pytest.raises(ValueError) as e:
            glue.filtfilt(torch.zeros(n, dtype=torch.float64), b, a)
        assert str(e.value) == str(e_ref.value)
    with pytest.raises(ValueError) as e:  # ... also for one item of a batch
        glue.filtfilt([torch.zeros(100, dtype=torch.float64), torch.zeros(18, dtype=torch.float64)], b, a)
    assert "padlen, which is 18" in str(e.value)
    for bb, aa in ((np.ones((2, 2)), a), (b, np.ones((2, 2)))):
        with pytest.raises(ValueError) as e_ref:
            signal.lfilter_zi(bb, aa)
        with pytest.raises(ValueError) as e:
            glue.lfilter_zi(bb, aa)
        assert str(e.value) == str(e_ref.value)
    with pytest.raises(ValueError):  # scipy divides by the zero and filters NaNs; there is nothing to compute
        glue.lfilter_zi(b, [0.0, 0.0])
    with pytest.raises(TypeError):
        glue.filtfilt(torch.zeros(100, dtype=torch.int16), b, a)
    with pytest.raises(ValueError):
        glue.filtfilt(torch.zeros(4, 100, dtype=torch.float64), b, a)
    with pytest.raises(ValueError):
        glue.filtfilt(torch.zeros(100, dtype=torch.float64), b, a, reflect_pad=100)


def test_a_cpu_tensor_is_refused_not_filtered_on_the_host():
    import rvc_amd
    from rvc_amd import glue

    b, a = FILTERS[0]
    with pytest.raises(rvc_amd.RvcmiError):
        glue.filtfilt(torch.zeros(1000, dtype=torch.float64), b, a)
    with pytest.raises(rvc_amd.RvcmiError):
        glue.highpass16k(torch.zeros(1000, dtype=torch.float32))


def test_highpass_coefficients_are_the_reference_modules():
    import types

    from rvc_amd import glue

    b, a = FILTERS[0]
    got = glue.highpass_coefficients()
    assert np.array_equal(got[0], b) and np.array_equal(got[1], a)
    assert np.array_equal(np.array(glue._HP16K[0]), b) and np.array_equal(np.array(glue._HP16K[1]), a)  # the no-scipy constants
    mod = types.SimpleNamespace(bh=np.array([1.0, -1.0]), ah=np.array([1.0, -0.5]))
    got = glue.highpass_coefficients(mod)
    assert np.array_equal(got[0], mod.bh) and np.array_equal(got[1], mod.ah)


def test_the_library_refuses_bad_arguments_before_any_launch():
    import rvc_amd

    L = rvc_amd._lib.lib()
    assert L.rvcmi_glue_filtfilt_scratch_bytes(2, 1000, 5) == (1000 + 2 * 18 * 2) * 8
    assert L.rvcmi_glue_filtfilt_scratch_bytes(0, 1000, 5) == 0 and L.rvcmi_glue_filtfilt_scratch_bytes(1, 1000, 9) == 0
    b = (C.c_double * 9)(*([1.0] * 9))
    a = (C.c_double * 9)(*([1.0] + [0.0] * 8))
    a_bad = (C.c_double * 9)(*([2.0] + [0.0] * 8))
    zi = (C.c_double * 8)()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused on its arguments
    P = lambda v: C.cast(v, C.c_void_p)  # noqa: E731

    def call(order=5, a_=a, B=1, max_len=1000, total=1000, warm=11264, pad=0, out_pad=None, scratch_bytes=1 << 20, x=fake):
        return L.rvcmi_glue_filtfilt(x, 1, fake, B, max_len, total, P(b), P(a_), P(zi), order, warm, fake, out_pad, pad, fake, scratch_bytes, None)

    for kw in (dict(order=0), dict(order=9), dict(a_=a_bad), dict(B=0), dict(max_len=18), dict(total=999), dict(warm=1000), dict(warm=-1024),
               dict(warm=(1 << 20) + 1024), dict(out_pad=fake, pad=1000), dict(scratch_bytes=8), dict(x=None)):
        assert call(**kw) == rvc_amd._lib.ERR_INVALID, kw


def test_the_fixture_inputs_regenerate_and_cover_what_the_issue_asks():
    from rvc_amd import glue

    names = prep_cases.names()
    kinds = {prep_cases.CASES[n][3] for n in names}
    assert {"plain", "zeros", "int16"} <= kinds and len(prep_cases.long_names()) >= 1
    short = [n for n in names if n not in prep_cases.long_names()]
    assert len(short) >= 3
    c = prep_cases.load(short[0])
    for n in short:
        secs = prep_cases.CASES[n][1] / 16000
        assert 3 <= secs <= 10 and prep_cases.CASES[n][1] // glue.FILT_LANE >= 8
    for n in prep_cases.long_names():
        assert prep_cases.CASES[n][1] >= 70 * 16000
    assert np.array_equal(c.b, FILTERS[0][0]) and np.array_equal(c.a, FILTERS[0][1])
    # scipy stays near the exact values at the stored positions (sanity of the fixture itself)
    assert np.abs(signal.filtfilt(c.b, c.a, c.x)[c.idx] - c.exact).max() < 1e-7
    z = prep_cases.load("zeros_stretch_7s").x
    assert (z[len(z) // 3: len(z) // 3 + 9000] == 0).all() and z.dtype == np.float32
    q = prep_cases.load("int16_quantised_4s").x.astype(np.float64) * 32768
    assert np.array_equal(q, np.rint(q))
