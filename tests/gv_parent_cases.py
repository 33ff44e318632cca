"""The trajectory conversions whose rows must not move now that conversion_trajectory can add the global-variance term
(DESIGN.md §12.2): without the term it must return what the commit before returned, bit for bit.

    INPUTS      tests/golden/gv_parent_inputs.npz: two dynamic maps and their source rows, stored so that every machine
                converts the same bits: `step_*`, mlpg_ref.step_case(), and `dyn_*`, the NumPy model's float64 map of
                mlpg_ref.dynamic_case() (six rounds) with that case's source rows CA
    cases()     name -> (conv dict, C): step, step_gap (row 100 empty), dynamic
    rows(amd, conv, C, **kw)   conversion_trajectory's result

Run as a program at the commit whose rows are to be kept, on the MI355X,

    python tests/gv_parent_cases.py <that commit's hash> [out.json]

it records shape + sha256 of the rows of every case in tests/golden/gv_parent_digests.json; tests/test_gpu_gv.py holds
every later conversion_trajectory without the term to them.  `python tests/gv_parent_cases.py --inputs` rebuilds the
inputs from the model on the host (no device)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "gv_parent_inputs.npz")
FIXTURE = os.path.join(HERE, "golden", "gv_parent_digests.json")
FIELDS = ("weights", "means", "covs", "zbar", "phi", "loglik", "n", "dx", "dy", "level", "A", "b", "Wx", "kx", "span", "py")


def write_inputs():
    import mlpg_ref as R
    step, C = R.step_case()
    CA, CB, X, Y, M, span = R.dynamic_case()
    f = R.train(X, Y, M, iters=6, tol=-1.0)
    dyn = dict(weights=f["weights"], means=f["means"], covs=f["covs"], zbar=f["zbar"], phi=f["phi"], loglik=f["loglik"],
               n=np.int64(f["n"]), dx=np.int64(f["dx"]), dy=np.int64(f["dy"]), level=np.bool_(f["level"]), A=f["A"], b=f["b"],
               Wx=np.tril(f["Wx"]), kx=f["kx"], span=np.int64(span), py=f["py"])
    out = dict(step_C=C, dyn_C=CA)
    for prefix, conv in (("step_", step), ("dyn_", dyn)):
        out.update({prefix + k: np.asarray(conv[k]) for k in FIELDS})
    np.savez_compressed(INPUTS, **out)


def cases():
    with np.load(INPUTS, allow_pickle=False) as z:
        step, dyn = ({k: z[p + k] for k in FIELDS} for p in ("step_", "dyn_"))
        C, CA = z["step_C"], z["dyn_C"]
    gap = C.copy()
    gap[100] = (-np.inf, 0.0)
    return dict(step=(step, C), step_gap=(step, gap), dynamic=(dyn, CA))


def rows(amd, conv, C, **kw):
    return amd.conversion_trajectory(conv, C, **kw)


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return dict(shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest())


def main(argv):
    if argv[1:] == ["--inputs"]:
        write_inputs()
        return 0
    sys.path.insert(0, os.path.dirname(HERE))
    import eaqhm_amd
    doc = dict(parent_commit=argv[1], digest="sha256 of the C-contiguous float64 bytes of conversion_trajectory(conv, C)",
               inputs="tests/golden/gv_parent_inputs.npz", cases={})
    for name, (conv, C) in cases().items():
        doc["cases"][name] = digest(rows(eaqhm_amd, conv, C))
    path = argv[2] if len(argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(doc["cases"]), path))
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
