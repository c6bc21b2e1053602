"""The one way a test sets the library's environment switches (flux_amd/csrc/flux_switches.h; DESIGN.md "Environment switches").
Setting some always clears the rest, so no test runs under a switch that another test, or the calling shell, left behind."""
import os

import pytest

NAMES = ("FLUX_SAMPLE_TABLES", "FLUX_THROUGHPUT_TABLE", "FLUX_LOBE_FRAMES", "FLUX_PLANE_AXIS", "FLUX_SAMPLE_ORDER",
         "FLUX_SPLIT_DEPTH_CUT", "FLUX_SPLIT_UNIFORM_A", "FLUX_SPLIT_HITQ_CAP", "FLUX_SPLIT_HITQ_TAKE_AT",
         "FLUX_DENOISE_LDS_LEVELS", "FLUX_BUILD_THREADS", "FLUX_RCCL_LIB")


def _checked(env):
    unknown = sorted(set(env) - set(NAMES))
    if unknown:
        raise KeyError(f"not a switch of the library: {', '.join(unknown)}")
    return env


def set_switches(monkeypatch, **env):
    """Set the given switches (str() of each value; None: unset) and unset every other one."""
    _checked(env)
    for name in NAMES:
        if env.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(env[name]))


def queue(q):
    """The hit queue's two switches for q = (cap, take_at); none for q = None."""
    return {} if q is None else {"FLUX_SPLIT_HITQ_CAP": q[0], "FLUX_SPLIT_HITQ_TAKE_AT": q[1]}


def clean_env(**more):
    """os.environ without any switch, plus `more` (None: nothing): the environment of a self-test's subprocess."""
    env = {k: v for k, v in os.environ.items() if k not in NAMES}
    env.update({k: str(v) for k, v in more.items() if v is not None})
    return env


@pytest.fixture
def switches(monkeypatch):
    """switches(**env): set_switches on this test's monkeypatch.  No switch is set before the first call or after the test."""
    def set_(**env):
        set_switches(monkeypatch, **env)
    set_()
    yield set_
    set_()
