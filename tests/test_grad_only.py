"""``bjx_target_diag_gaussian_grad`` (the gradient-only launch of an HMC trajectory's intermediate evaluations): argument
checking happens before any device work, so it is testable without a GPU, like ``test_abi.test_error_reporting_without_gpu``
for the leapfrog."""
import ctypes

NAME = b"bjx_target_diag_gaussian_grad"


def _lib():
    from blackjax_amd import _lib

    return _lib.load()


def test_grad_entry_point_is_bound_with_the_declared_prototype():
    from blackjax_amd import _lib

    assert len(_lib.SIGNATURES["bjx_target_diag_gaussian_grad"]) == 6  # stream, N, D, inv_var, q, g_out
    assert _lib.load().bjx_abi_version() == 7  # an additive change: the ABI number stays


def test_grad_entry_point_rejects_null_pointers():
    lib = _lib()
    buf = (ctypes.c_float * 8)()
    ok = ctypes.addressof(buf)
    for args in ((None, ok, ok), (ok, None, ok), (ok, ok, None), (None, None, None)):
        rc = lib.bjx_target_diag_gaussian_grad(None, 2, 4, *args)
        assert rc != 0 and NAME in lib.bjx_last_error()


def test_grad_entry_point_rejects_bad_sizes():
    lib = _lib()
    buf = (ctypes.c_float * 8)()
    ok = ctypes.addressof(buf)
    for n, d in ((2, 0), (2, -4), (-1, 4)):
        rc = lib.bjx_target_diag_gaussian_grad(None, n, d, ok, ok, ok)
        assert rc != 0 and NAME in lib.bjx_last_error()


def test_grad_entry_point_accepts_an_empty_batch():
    assert _lib().bjx_target_diag_gaussian_grad(None, 0, 4, None, None, None) == 0


def test_generated_targets_carry_gradient_only_kernels():
    """The hiprtc units of ``DeviceTarget`` / ``ElementwiseRowsTarget`` (cross-compiled: no GPU needed) export the
    gradient-only kernels next to the full ones."""
    import torch

    import blackjax_amd as bjx
    from blackjax_amd import elementwise, rtc
    from test_device_target import QUARTIC

    code = bjx.targets.DeviceTarget(QUARTIC).code_object()
    for ni in (1, 2, 4):
        assert b"bjx_rtc_grad_%d" % ni in code and b"bjx_rtc_eval_%d" % ni in code
    src = elementwise.trace(lambda q: -0.5 * (q * q).sum(-1) - torch.nn.functional.softplus(q).sum(-1), 1500)
    code = rtc.compile(elementwise.ROWS_TU % {"source": src.rows_source}, "bjx_elementwise_rows.hip")
    assert b"bjx_rtc_ew_grad_rows" in code and b"bjx_rtc_ew_rows" in code
