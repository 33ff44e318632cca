"""The fits that must not move now that gmm_fit and conversion_train can start from a k-means codebook:
with init=None they must return what the commit before returned, bit for bit.

    cases()     name -> the call: `fit`, gmm_fit on the joint rows of gmm_ref's sep_600x3 (M = 3, 6 rounds, split = 3),
                and `train_span2`, conversion_train(span=2) on seeded clustered rows of 2 x 3 columns a side (M = 2)
    digest(d)   shape + sha256 of the float64 bytes of the result's array fields, in FIELDS' order

Run as a program at the commit whose results are to be kept, on the MI355X,

    python tests/kmeans_parent_cases.py <that commit's hash> [out.json] [root of that commit's checkout]

it records the digests in tests/golden/kmeans_parent_digests.json; tests/test_gpu_kmeans.py holds every later
gmm_fit(init=None) and conversion_train(init=None, span=2) to them."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kmeans_parent_digests.json")
FIELDS = ("weights", "means", "covs", "zbar", "phi", "loglik", "A", "b", "Wx", "kx", "py")


def cases():
    import gmm_ref as G
    X, Y, _, M = G.case("sep_600x3")
    Xd, Yd, _ = G.clustered(500, 6, 2, 8.0, 0.05, 21)
    return dict(fit=lambda amd: amd.gmm_fit(np.hstack((X, Y)), M, iters=6, tol=0.0, init=None, split=3),
                train_span2=lambda amd: amd.conversion_train(Xd, Yd, 2, iters=6, tol=0.0, init=None, span=2))


def digest(result):
    h, shapes = hashlib.sha256(), {}
    for name in FIELDS:
        if name in result:
            a = np.ascontiguousarray(result[name], dtype=np.float64)
            shapes[name] = list(a.shape)
            h.update(a.tobytes())
    return dict(shapes=shapes, sha256=h.hexdigest())


def main(argv):
    sys.path.insert(0, argv[3] if len(argv) > 3 else os.path.dirname(HERE))
    import eaqhm_amd
    doc = dict(parent_commit=argv[1], digest="sha256 of the C-contiguous float64 bytes of the fields %s that the result "
               "has, in that order" % ", ".join(FIELDS), cases={})
    for name, call in cases().items():
        doc["cases"][name] = digest(call(eaqhm_amd))
    path = argv[2] if len(argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s (package: %s)" % (len(doc["cases"]), path, os.path.dirname(eaqhm_amd.__file__)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
