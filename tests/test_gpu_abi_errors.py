"""Entry points of the C ABI that refuse a call AFTER they hold device memory, and what the same context or scene does next: the LDS
budget of flux_debug_shade and of the render calls (STRICT keeps 32 B of recursion stack per level and lane: 64 lanes at depth 40 are
81 920 B, launch_plan.cpp lane_stacks_lds), an undersized output of flux_ctx_copy_table, and a flux_multi_create that fails.  A refusal
must leave nothing behind that the next call trips over: the context renders the bits of a fresh one afterwards."""
import ctypes as C

import numpy as np
import pytest

from conftest import small_scene

pytestmark = pytest.mark.gpu

DEPTH = 40  # 40 levels * 32 B * 64 lanes > 64 KiB


@pytest.fixture(scope="module")
def job(flux, demo1):
    return small_scene(demo1, 40, 30), flux.JobConfiguration(8, DEPTH, 50)


def _rays():
    o = np.tile([0.0, 2.0, -10.0], (5, 1))
    d = np.array([[0.0, -0.1, 1.0], [0.2, -0.1, 1.0], [-0.2, 0.0, 1.0], [0.0, 0.3, 1.0], [0.1, -0.3, 1.0]])
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def test_lds_refusals_leave_the_context_usable(flux, job):
    sd, cfg = job
    o, d = _rays()
    with flux.Renderer(sd, cfg, seed=5) as fresh:
        want = fresh.render_rows(0, 29)
    with flux.Renderer(sd, cfg, seed=5) as r:
        r.set_math(flux._lib.MATH_STRICT)
        with pytest.raises(flux.FluxError, match="64 KiB") as ex:
            r.debug_shade(o, d, depth=5)
        assert ex.value.code == flux._lib.E_INVALID
        with pytest.raises(flux.FluxError, match="64 KiB") as ex:
            r.render_rows(0, 0)
        assert ex.value.code == flux._lib.E_INVALID
        r.set_math(flux._lib.MATH_FAST)
        first = r.debug_shade(o, d, depth=5)
        second = r.debug_shade(o, d, depth=5)
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
        assert (first[1] >= 0).any() and np.isfinite(first[0]).all()
        assert np.array_equal(r.render_rows(0, 29), want)


@pytest.mark.parametrize("which", ["TABLE_HEMI", "TABLE_PIXEL"])
def test_undersized_table_output_is_refused(flux, job, which):
    sd, cfg = job
    lib = flux._lib.lib
    which = getattr(flux._lib, which)
    with flux.Renderer(sd, cfg, seed=5) as r:
        want = r.table(which)
        out = np.full(want.size, -1.0)
        dp = out.ctypes.data_as(C.POINTER(C.c_double))
        for short in (want.size - 1, 0):
            assert lib.flux_ctx_copy_table(r._handle(), which, dp, short) == flux._lib.E_INVALID
            assert "output too small" in flux._lib.last_error()
        assert (out == -1.0).all()
        assert lib.flux_ctx_copy_table(r._handle(), which, dp, out.size) == 0
        assert np.array_equal(out.reshape(want.shape), want)
        assert np.abs(want).max() <= 1.0 and np.abs(want).max() > 0.5


def test_a_refused_multi_renderer_leaves_the_device_usable(flux, demo1):
    sd = small_scene(demo1, 40, 30)
    cfg = flux.JobConfiguration(4, 5, 50)
    loop = flux._lib.SHARD_LOOPBACK
    with pytest.raises(flux.FluxError, match="sample_root"):
        flux.MultiRenderer(sd, cfg, seed=2, devices=[0, 0], shard=flux.SHARD_SETS | loop)
    # a refusal behind the argument checks: the flux_multi and its ranks exist by then, no rank has a context yet
    with pytest.raises(flux.FluxError, match="max_trace_depth"):
        flux.MultiRenderer(sd, flux.JobConfiguration(4, 300, 50), seed=2, devices=[0, 0], shard=loop)
    with flux.Renderer(sd, cfg, seed=2) as r:
        want = r.render_frame()
    with flux.MultiRenderer(sd, cfg, seed=2, devices=[0, 0], shard=loop) as m:
        assert m.info()["devices"] == 2
        assert np.array_equal(m.render_frame(), want)
