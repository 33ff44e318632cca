"""The interpolation-stage cases whose outputs must not move when eaqhm_spline_kernel and eaqhm_eval_kernel are
restructured (csrc/eaqhm_interp.hip: blocks on the knot grid, record rows through LDS): the eleven generated cases of
interp_stage_ref.cases() and small geometry cases around every block size the evaluation can choose.

    all_cases()            the eleven, then GEOMETRY
    GEOMETRY               No_ti = 40, Kmax = 12, lengths = SHORT at steps 1, 2, 7, 15, 16, 31, 32, 33, 63, 64, 65 and 80,
                           each without and with `extra = step` samples past the last instant; Kmax = 120 at step 15
    outputs(stage)         dict(name -> array) of one whole-range run of a test_gpu_interp_stage.Stage: code, mom, am,
                           fm, ph_knot, s_hat and the eight limbs (int64)

Run as a program at the commit whose outputs are to be kept, on the MI355X,

    python tests/interp_parent_cases.py <that commit's hash> [out.json]

it records shape + sha256 of every output of every case in tests/golden/interp_parent_digests.json;
tests/test_gpu_interp_parent.py holds every later library to them."""
import hashlib
import json
import os
import sys

import numpy as np

import interp_stage_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "interp_parent_digests.json")
STEPS = (1, 2, 7, 15, 16, 31, 32, 33, 63, 64, 65, 80)
FS = 16000


def geometry_cases():
    out = []
    for step in STEPS:
        for extra in (0, step):
            out.append(R.make_case("g_s%d_k12%s" % (step, "_past" if extra else ""), 40, 12, step, FS, extra=extra,
                                   lengths=R.SHORT))
    out.append(R.make_case("g_s15_k120", 40, 120, 15, FS, lengths=R.SHORT))
    return out


GEOMETRY = geometry_cases()


def all_cases():
    return R.cases() + GEOMETRY


def outputs(stage):
    got = stage.evaluate()
    out = dict(code=stage.code.cpu().numpy(), mom=stage.mom.cpu().numpy())
    for key in ("am", "fm", "ph_knot", "s_hat"):
        out[key] = got[key]
    out["limbs"] = np.array(got["limbs"], dtype=np.int64)
    return out


def digest(a):
    a = np.ascontiguousarray(a)
    return dict(shape=list(a.shape), dtype=str(a.dtype), sha256=hashlib.sha256(a.tobytes()).hexdigest())


def main(argv):
    sys.path.insert(0, os.path.dirname(HERE))
    from eaqhm_amd.functions import _ctx
    from test_gpu_interp_stage import Stage
    ctx = _ctx(0)
    doc = dict(parent_commit=argv[1], digest="sha256 of the C-contiguous bytes (float64; code uint8; limbs int64)",
               cases={})
    for case in all_cases():
        doc["cases"][case["name"]] = {k: digest(v) for k, v in outputs(Stage(ctx, case)).items()}
    path = argv[2] if len(argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(doc["cases"]), path))
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
