"""The Python surface of the model layer (no GPU, no library load): the public names of `eaqhm_amd` and of
`eaqhm_amd.model`, their signatures and docstrings, against tests/golden/python_api.json, the same for
`eaqhm_amd.convert` against tests/golden/python_api_convert.json, and the import order of the modules behind model.py
and behind convert.py.

The fixture was recorded from the commit before model.py was split, from the repository root, by

    import hashlib, inspect, json, eaqhm_amd
    from eaqhm_amd import model
    def entry(v):
        if not callable(v):
            return {"repr": repr(v)}
        try:
            sig = str(inspect.signature(v))
        except ValueError:                       # an exception class without an __init__ of its own
            sig = None
        return {"signature": sig, "doc": hashlib.sha256((v.__doc__ or "").encode()).hexdigest()}
    own = lambda v: not inspect.ismodule(v) and (not callable(v) or v.__module__.startswith("eaqhm_amd"))
    api = {m.__name__: {n: entry(v) for n, v in vars(m).items() if not n.startswith("_") and own(v)}
           for m in (eaqhm_amd, model)}
    json.dump(api, open("tests/golden/python_api.json", "w"), indent=1, sort_keys=True)

Submodules and what a module merely imports from outside the package (np, itertools.chain, ..) are not part of the
surface.  A change of the surface on purpose re-records the fixture with the same script."""
import hashlib
import inspect
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT

PACKAGE = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
LAYERS = ("args", "records", "cepstrum", "align", "noise", "model")     # each imports only from the ones before it
ALLOWED = {m: set(LAYERS[:i + 1]) for i, m in enumerate(LAYERS)}
# the conversion branches off after align: neither noise nor model
CONVERT_LAYERS = ("args", "records", "cepstrum", "align", "mixture", "dynamics", "mapping", "convert", "nonparallel")
ALLOWED.update({m: set(CONVERT_LAYERS[:i + 1]) for i, m in enumerate(CONVERT_LAYERS) if i >= 4})

# `import eaqhm_amd.<m>` runs the package's __init__ first, which imports model before anything else; so <m> is also
# imported under a bare package (the directory on __path__, no __init__): then it is the first module of the package to
# load, and what it pulls in is what its own import lines ask for.
FIRST = ("import importlib, sys, types; p = types.ModuleType('eaqhm_amd'); p.__path__ = [%r]; "
         "sys.modules['eaqhm_amd'] = p; importlib.import_module('eaqhm_amd.%s'); "
         "print(' '.join(sorted(k[10:] for k in sys.modules if k.startswith('eaqhm_amd.'))))")


def _entry(v):
    if not callable(v):
        return {"repr": repr(v)}
    try:
        sig = str(inspect.signature(v))
    except ValueError:
        sig = None
    return {"signature": sig, "doc": hashlib.sha256((v.__doc__ or "").encode()).hexdigest()}


def _own(v):
    return not inspect.ismodule(v) and (not callable(v) or v.__module__.startswith("eaqhm_amd"))


def test_public_surface_is_the_recorded_one():
    import eaqhm_amd
    from eaqhm_amd import model
    with open(os.path.join(GOLDEN, "python_api.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == ["eaqhm_amd", "eaqhm_amd.model"]
    for m in (eaqhm_amd, model):
        now = {n: _entry(v) for n, v in vars(m).items() if not n.startswith("_") and _own(v)}
        want = recorded[m.__name__]
        assert sorted(now) == sorted(want), (m.__name__, set(now) ^ set(want))
        changed = [n for n in want if now[n] != want[n]]
        assert not changed, (m.__name__, changed)
    surface = recorded["eaqhm_amd.model"].values()
    assert sum("repr" in e for e in surface) == 14 and sum("signature" in e for e in surface) == 67


def test_convert_surface_is_the_recorded_one():
    """eaqhm_amd.convert against tests/golden/python_api_convert.json, recorded by the script above applied to convert,
    from the commit before convert.py was split by layer; "underscore" lists that commit's single-underscore names, which
    all stay attributes of convert.  "added" and "added_underscore" were written in by hand: what the split itself added."""
    from eaqhm_amd import convert
    with open(os.path.join(GOLDEN, "python_api_convert.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == ["added", "added_underscore", "eaqhm_amd.convert", "underscore"]
    surface = recorded["eaqhm_amd.convert"]
    assert len(surface) == 59 and sum("signature" in e for e in surface.values()) == 39
    assert sum("repr" in e for e in surface.values()) == 20 and len(recorded["underscore"]) == 18
    assert sorted(recorded["added"]) == ["mlpg_work_len"] and not set(recorded["added"]) & set(surface)
    now = {n: _entry(v) for n, v in vars(convert).items() if not n.startswith("_") and _own(v)}
    want = dict(surface, **recorded["added"])
    assert sorted(now) == sorted(want), set(now) ^ set(want)
    changed = [n for n in want if now[n] != want[n]]
    assert not changed, changed
    missing = [n for n in recorded["underscore"] + recorded["added_underscore"] if not hasattr(convert, n)]
    assert not missing, missing


def test_each_module_imports_first():
    """Every module imported in an interpreter of its own, twice: by `import eaqhm_amd.<m>`, and first of the package.
    The interpreters run side by side."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda code: subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                        stderr=subprocess.PIPE, text=True)
    procs = {m: (run("import eaqhm_amd.%s" % m), run(FIRST % (PACKAGE, m))) for m in ALLOWED}
    for m, (whole, first) in procs.items():
        _, err = whole.communicate()
        assert whole.returncode == 0, (m, err)
        out, err = first.communicate()
        assert first.returncode == 0, (m, err)
        loaded = set(out.split())
        assert m in loaded and loaded <= ALLOWED[m], (m, loaded - ALLOWED[m])
