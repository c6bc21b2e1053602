"""tests/split_checks.py against a stub library: a Renderer and an Oracle that return canned arrays and log their calls.  No GPU and
no built library."""
import types

import numpy as np
import pytest

import split_checks as sc
import switches


class _Renderer:
    def __init__(self, log, sd, cfg, seed):
        self.log, self.counting = log, False
        log.append(("open", sd, cfg, seed))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.log.append(("close",))

    def set_kernel(self, kernel):
        self.log.append(("kernel", kernel))

    def enable_stats(self, on):
        self.counting = on

    def stats(self, reset=False):
        return {"samples": 7}

    def render_frame(self):
        self.log.append(("frame", self.counting))
        return np.full((2, 3, 3), 1.0 if self.counting else 2.0)

    def launch_plan(self, flags=False):
        return {"kernel": 3, **({"flags": 5} if flags else {})}

    def device_bytes(self):
        return 4096


class _Oracle:
    def __init__(self, log, sd, cfg, seed):
        self.log = log
        log.append(("oracle", sd, cfg, seed))

    def stats(self, reset=False):
        self.log.append(("oracle stats", reset))
        return {"samples": 7}

    def render_frame(self, threads):
        self.log.append(("oracle frame", threads))
        return np.zeros((2, 3, 3))

    def close(self):
        self.log.append(("oracle close",))


@pytest.fixture
def stub():
    log = []
    flux = types.SimpleNamespace(KERNEL_STATIC=1, KERNEL_REFILL=2, KERNEL_SPLIT=3, JobConfiguration=lambda *a: a,
                                 Renderer=lambda sd, cfg, seed: _Renderer(log, sd, cfg, seed))
    oracle_mod = types.SimpleNamespace(Oracle=lambda sd, cfg, seed: _Oracle(log, sd, cfg, seed))
    return flux, oracle_mod, log


def _frames(log):
    return [entry[1] for entry in log if entry[0] == "frame"]


def test_render_launches_one_frame_or_the_plain_one_first(stub):
    flux, _, log = stub
    run = sc.render(flux, "scene", 16, 5, 4, kernel=flux.KERNEL_SPLIT)
    assert _frames(log) == [True] and run.plain is None
    assert log[:2] == [("open", "scene", (16, 5, 50), 4), ("kernel", 3)] and log[-1] == ("close",)
    assert run.frame[0, 0, 0] == 1.0 and run.stats == {"samples": 7} and run.plan == {"kernel": 3} and run.device_bytes == 4096
    del log[:]
    run = sc.render(flux, "scene", 16, 5, 4, plain=True)
    assert _frames(log) == [False, True] and run.plain[0, 0, 0] == 2.0 and run.frame[0, 0, 0] == 1.0
    assert not any(entry[0] == "kernel" for entry in log)   # none given: the plan's own


def test_split_run_renders_without_statistics_first(stub):
    flux, _, log = stub
    with flux.Renderer("scene", None, 1) as r:
        r.enable_stats(True)
        plain, frame, stats, plan = sc.split_run(flux, r)
    assert _frames(log) == [False, True] and ("kernel", flux.KERNEL_SPLIT) in log
    assert plain[0, 0, 0] == 2.0 and frame[0, 0, 0] == 1.0 and plan["flags"] == 5


def test_oracle_run_resets_and_closes(stub):
    flux, oracle_mod, log = stub
    frame, stats = sc.oracle_run(flux, oracle_mod, "scene", 16, 5, 4)
    assert log == [("oracle", "scene", (16, 5, 50), 4), ("oracle stats", True), ("oracle frame", 8), ("oracle stats", False),
                   ("oracle close",)]
    assert not frame.flags.writeable and stats == {"samples": 7}


def test_references_are_made_once_a_key_and_read_only(stub):
    flux, oracle_mod, log = stub
    cache = {}
    first = sc.references(cache, "a", flux, oracle_mod, "scene", 16, 5, 4, oracle_sd="the oracle's scene")
    made = list(log)
    assert sc.references(cache, "a", flux, oracle_mod, "scene", 16, 5, 4) is first and log == made
    want, o_stats, refill, static = first
    assert [entry[1] for entry in log if entry[0] in ("oracle", "open", "kernel")] == ["the oracle's scene", "scene", 2, "scene", 1]
    assert _frames(log) == [True, True]
    for a in (want, refill.frame, static.frame):
        assert not a.flags.writeable
    # another key is another run; no oracle scene, one kernel
    del log[:]
    want, o_stats, static = sc.references(cache, "b", flux, oracle_mod, "scene", 16, 5, 4, oracle_sd=None, kernels=("STATIC",))
    assert want is None and o_stats is None and _frames(log) == [True] and not any(entry[0] == "oracle" for entry in log)
    assert sc.references(cache, "c", flux, oracle_mod, "scene", 16, 5, 4, kernels=())[1] == {"samples": 7}
    assert sorted(cache) == ["a", "b", "c"]


@pytest.mark.parametrize("name", switches.NAMES)
def test_references_refuse_an_environment_with_a_switch(stub, monkeypatch, name):
    flux, oracle_mod, log = stub
    monkeypatch.setenv(name, "0")
    with pytest.raises(AssertionError):
        sc.references({}, "a", flux, oracle_mod, "scene", 16, 5, 4)
    assert log == []


def test_same_bits_is_about_bits():
    a = np.array([0.0, 1.0, np.nan])
    assert sc.same_bits(a, a.copy())
    assert not sc.same_bits(np.array([0.0]), np.array([-0.0]))
    other_nan = a.copy()
    other_nan.view(np.uint64)[2] ^= 1   # another payload
    assert np.isnan(other_nan[2]) and np.array_equal(a, other_nan, equal_nan=True) and not sc.same_bits(a, other_nan)
    assert not sc.same_bits(np.zeros(4), np.zeros((2, 2)))


def test_distance_is_over_the_pixels_finite_in_both():
    a = np.array([1.0, np.inf, np.nan, 2.0])
    b = np.array([1.5, np.nan, -np.inf, 2.0])
    assert sc.distance(a, b) == 0.5
    assert sc.distance(np.array([np.nan]), np.array([np.inf])) == 0.0
    with pytest.raises(AssertionError, match="finiteness"):
        sc.distance(a, np.array([1.0, 3.0, np.nan, 2.0]))


def test_turns_take_the_floor_normal_to_the_axis_in_the_name():
    axes = {"plus_x": (1, 0, 0), "minus_x": (-1, 0, 0), "plus_y": (0, 1, 0), "minus_y": (0, -1, 0), "plus_z": (0, 0, 1),
            "minus_z": (0, 0, -1)}
    assert list(sc.TURNS) == ["plus_y", "minus_y", "plus_x", "minus_x", "plus_z", "minus_z"]
    for name, turn in sc.TURNS.items():
        assert turn((0, 1, 0)) == axes[name]
        m = np.array([turn(e) for e in np.eye(3)])
        assert round(float(np.linalg.det(m))) == 1   # a rotation: no mirror image
