"""What tests/test_gpu_pass_fuzz.py rests on, from the references alone: for every generated scene of the default chunks the pinned
τ keeps the adaptive run's decision margin >= 1e-9 and its path margin >= 1e-10 -- so the kernels' pass map must be EQUAL --, at
least half of the pass maps are not constant, a NaN pixel is never hot, and only scenes with non-unit normals have non-finite
sample radiance, so that the comparison that tolerates a non-finite reference is used nowhere else.  No GPU."""
import numpy as np
import pytest

import moments_spec as ms
import test_gpu_ext_fuzz as ext
import test_gpu_pass_fuzz as pf

DEFAULT_CHUNKS = [(False, c) for c in range(12)] + [(True, c) for c in range(4)]


def test_the_table_covers_the_default_chunks():
    assert [(mesh, len(rows)) for mesh, rows in pf.TAU.items()] == [(False, 12), (True, 4)]
    assert all(len(row) == ext.CASES and set(row) <= set(pf.LADDER) for rows in pf.TAU.values() for row in rows)
    assert pf.ADAPTIVE["max_passes"] <= 8   # the narrowest frame the generator draws: no set is read twice


@pytest.mark.parametrize("mesh,chunk", DEFAULT_CHUNKS)
def test_pinned_thresholds_keep_the_margins(flux, mesh, chunk):
    for case, (sd, n, D, seed, spec) in enumerate(ext.chunk_references(chunk, mesh)):
        par, res = pf.adaptive_reference(mesh, chunk, case)
        hist = np.bincount(res.passes.ravel()).tolist()
        print(f"pass fuzz {'mesh ' if mesh else ''}chunk {chunk} case {case}: {res.passes.shape[1]} x {res.passes.shape[0]}, n {n}, D {D}, tau "
              f"{par['threshold']}, rounds {len(res.active)}, pass histogram {hist}, decision margin {res.decision_margin:.2e}, path margin "
              f"{res.path_margin:.2e}")
        assert par["threshold"] == pf.TAU[mesh][chunk][case] and par["max_passes"] == 4 and par["dilate"] == 1
        assert res.decision_margin >= pf.DECISION_MARGIN, (mesh, chunk, case)
        assert res.path_margin >= ms.MIN_MARGIN, (mesh, chunk, case)
        assert res.passes.shape == (sd.output_settings.image_height, sd.output_settings.image_width)
        assert res.passes.min() >= 1 and res.passes.max() <= 4 and par["max_passes"] <= spec.width
        nan = np.isnan(res.sums[..., 3]) | np.isnan(res.sums[..., 4])
        for hot in res.hot:   # a NaN pixel is never hot: alone it stops after min_passes
            assert not hot[nan].any()
        if nan.all():
            assert np.all(res.passes == par["min_passes"])
        # one pass of the rule is the scene's sample moments
        if len(res.active) == 1:
            assert np.array_equal(res.moments, pf.moments_reference(mesh, chunk, case), equal_nan=True)


def test_at_least_half_of_the_pass_maps_are_not_constant():
    varied = sum(len(np.unique(pf.adaptive_reference(mesh, chunk, case)[1].passes)) > 1
                 for mesh, chunk in DEFAULT_CHUNKS for case in range(ext.CASES))
    print(f"pass fuzz: {varied} of {len(DEFAULT_CHUNKS) * ext.CASES} pass maps are not constant")
    assert varied >= 32


def test_only_scenes_with_non_unit_normals_have_non_finite_samples(flux):
    odd = set()
    for mesh, chunk in DEFAULT_CHUNKS:
        for case, (sd, n, D, seed, spec) in enumerate(ext.chunk_references(chunk, mesh)):
            assert spec.sample_radiance.shape == (sd.output_settings.image_height, sd.output_settings.image_width, n * n, 3)
            if not np.isfinite(spec.sample_radiance).all():
                assert ext.non_unit_normal(flux, sd), (mesh, chunk, case)
                odd.add((mesh, chunk, case))
            want = pf.moments_reference(mesh, chunk, case)
            assert np.isfinite(want).all() == ((mesh, chunk, case) not in odd)
            assert np.array_equal(want[..., ms.RGB], spec.frame(), equal_nan=True)   # (as tests/test_moments.py shows for its scenes)
    assert odd == pf.NON_FINITE
    # two of the three hold finite and non-finite pixels side by side, so the masked comparison judges both kinds
    mixed = [k for k in sorted(odd) if np.isfinite(pf.moments_reference(*k)).all(axis=2).any()]
    assert len(mixed) == 2, mixed
