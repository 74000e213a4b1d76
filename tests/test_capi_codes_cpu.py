"""CPU only: every launching C-ABI entry point returns today what tests/golden/capi_codes.json recorded from the commit before the
argument checks were last rearranged -- for the valid base call, every single bad argument and every PAIR of bad arguments, which
is what pins the code that wins when two things are wrong at once (tools/record_capi_codes.py: the grid, and how to record).

Only the held cases are replayed: those whose recorded code is a validation code.  A '.' case reached HIP when it was recorded
and is never called here.  The test SKIPS where a GPU is visible: it checks host code, and if a regression let a held case
through validation, the call would launch on the grid's made-up pointers."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT, pkg


def _tool():
    spec = importlib.util.spec_from_file_location("record_capi_codes", os.path.join(ROOT, "tools", "record_capi_codes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "capi_codes.json")) as f:
        return json.load(f)


def test_fixture_covers_every_launching_entry_point(recorded):
    """the fixture names exactly the header's prototypes with a hip_stream parameter, parameter by parameter, and holds enough"""
    tool = _tool()
    with open(os.path.join(ROOT, "include", "fr_hotpath.h")) as f:
        eps = tool.entry_points(f.read())
    funcs = recorded["functions"]
    assert len(eps) == 32 and [name for name, _ in eps] == list(funcs)
    for name, names in eps:
        assert funcs[name]["params"].split() == names, name
    assert recorded["grid"] == tool.GRID
    total = sum(len(v["codes"]) for v in funcs.values())
    held = total - sum(v["codes"].count(".") for v in funcs.values())
    assert held >= 0.8 * total, (held, total)
    for name, v in funcs.items():
        assert len(v["codes"]) - v["codes"].count(".") >= 0.6 * len(v["codes"]), name
        assert {"0", "1"} <= set(v["codes"]) <= set("0124."), name


def test_every_held_return_code_is_unchanged(recorded):
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    tool = _tool()
    host = pkg("_lib")
    L = host.lib()
    want_of = {ch: code for code, ch in tool.CHARS.items()}
    replayed, wrong = 0, []
    for name, v in recorded["functions"].items():
        f = getattr(L, name)
        calls = list(tool.cases(name, v["params"].split(), host.SIGNATURES[name], recorded["grid"]))
        assert len(calls) == len(v["codes"]), name
        for k, (args, ch) in enumerate(zip(calls, v["codes"])):
            if ch == ".":
                continue
            replayed += 1
            got = f(*args)
            if got != want_of[ch]:
                wrong.append((name, k, [getattr(a, "value", a) for a in args], want_of[ch], got))
    print("replayed %d held cases of %d entry points" % (replayed, len(recorded["functions"])))
    assert not wrong, "%d of %d held cases changed their code; the first: %r" % (len(wrong), replayed, wrong[:5])
