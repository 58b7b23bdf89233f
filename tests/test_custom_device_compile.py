"""CPU: caller-defined Transformation hooks as device source (include/vsom_hip.h, vsom_create_custom) compile for gfx950
through vsom_custom_compile_check, which opens no device.  The three built-ins restated as source compile; a source
with a syntax error, an empty source and a depth beyond VSOM_CUSTOM_MAX_DEPTH are refused with VSOM_ERR_INVALID."""
import pytest

from vsom_amd import capi

import custom_hooks as hooks

INVALID = -1


def _check(source, depth, residual_len):
    L = capi.lib()
    return L.vsom_custom_compile_check(source.encode(), depth, residual_len), L.vsom_last_error().decode(errors="replace")


@pytest.mark.parametrize("kind", ["standard", "median", "clr"])
def test_builtins_restated_as_source_compile(kind):
    depth, rlen = hooks.shape(kind, 9)
    rc, err = _check(hooks.SOURCES[kind], depth, rlen)
    assert rc == 0, err


def test_non_builtin_hook_compiles():
    capi.custom_compile_check(hooks.SIGMA_NORMALISED, 13, 13)


def test_syntax_error_returns_invalid_with_the_hiprtc_log():
    bad = hooks.STANDARD.replace("return x[d] - model[d];", "return x[d] - model[d]")
    rc, err = _check(bad, 9, 9)
    assert rc == INVALID
    assert "does not compile" in err
    assert "error" in err and "hook_source" in err      # the hipRTC diagnostic, located in the caller's source
    with pytest.raises(capi.VsomError):
        capi.custom_compile_check(bad, 9, 9)


def test_missing_hook_is_a_compile_error():
    only_compare = hooks.STANDARD[:hooks.STANDARD.index("__device__ float vsom_step")]
    rc, err = _check(only_compare, 9, 9)
    assert rc == INVALID and "vsom_step" in err


def test_refused_shapes():
    assert _check("", 9, 9)[0] == INVALID
    assert _check(hooks.STANDARD, 0, 9)[0] == INVALID
    assert _check(hooks.STANDARD, 9, 0)[0] == INVALID
    rc, err = _check(hooks.STANDARD, capi.CUSTOM_MAX_DEPTH + 1, 9)
    assert rc == INVALID and "VSOM_CUSTOM_MAX_DEPTH" in err
    assert _check(hooks.STANDARD, capi.CUSTOM_MAX_DEPTH, 9)[0] == 0


def test_no_device_means_no_custom_context():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.VsomError):
        capi.Context(4, 4, 3, capi.CUSTOM, source=hooks.STANDARD, depth=3, residual_len=3)
