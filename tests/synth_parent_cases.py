"""The resynthesis cases whose samples must not move when the synthesis entry points are folded (ABI 6): every arm of
the dispatch behind eaQHMSynthesis and eaQHMNoiseSynthesis, through the public API only, on the committed SA19 model
(tests/golden/sa19_female_default.npz) and the residual of tests/golden/SA19.WAV against the fixture's s_recon.

    cases(amd, inputs(amd)) -> dict(name -> float64 array)

  1. eaQHMSynthesis, phase in {independent, shape} x map in {scalar (rho, beta) = (0.5, 1.25), contour rho = 0.9 + 0.4 x,
     beta = 1.3 - 0.5 x}, each whole and ("_ranges") in three uneven ranges whose bounds are multiples of neither 64 nor
     the step; phase="shape" with an explicit f0 (model_f0 x 0.9) on the scalar map.
  2. eaQHMNoiseSynthesis at noise_time_map for rho in {0.5, 2}, without and with fundamental=noise_fundamental(...),
     each whole and in three ranges whose bounds are no multiples of the hop.
  3. eaQHMSynthesis(noise=...) on the scalar map with phase="shape" and on the contour map with phase="independent",
     each with the plain noise and with noise_modulation=True, noise_formant=True, formant_scale=1.2.

Run as a program at the commit whose samples are to be kept, on the MI355X,

    python tests/synth_parent_cases.py <that commit's hash> [out.json]

it records shape + sha256 of every case in tests/golden/synth_parent_digests.json; tests/test_gpu_synth_parent.py holds
every later library to them."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "synth_parent_digests.json")
FS = 16000
SCALAR = (0.5, 1.25)
RANGES = "_ranges"


def contours(n):
    x = np.arange(n) / (n - 1)
    return 0.9 + 0.4 * x, 1.3 - 0.5 * x


def split(L_out, *avoid):
    """Three uneven ranges covering [0, L_out): the two inner bounds are multiples of none of `avoid`."""
    cuts = []
    for c in (L_out // 5, (2 * L_out) // 3):
        while any(c % m == 0 for m in avoid):
            c += 1
        cuts.append(c)
    assert 0 < cuts[0] < cuts[1] < L_out
    return [(0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], L_out)]


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return dict(shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest())


def inputs(amd):
    """(det, L, step, noise model with mod) of the committed SA19 fixture."""
    from test_gpu_model_synthesis import reference_model
    g, det = reference_model()
    fs, s = amd.read_signal(os.path.join(HERE, "golden", "SA19.WAV"))
    s_recon = np.asarray(g["s_recon"], dtype=np.float64)
    assert fs == FS and len(s) == len(s_recon)
    nz = amd.eaQHMNoiseModulation(s, s_recon, amd.eaQHMNoiseAnalysis(s, s_recon, fs), det)
    return det, len(s), int(det["ti"][1] - det["ti"][0]), nz


def cases(amd, inp):
    from eaqhm_amd.model import contour_time_map, noise_time_map
    det, L, step, nz = inp
    n = len(det["ti"])
    rho_c, beta_c = contours(n)
    maps = dict(scalar=(dict(time_scale=SCALAR[0], pitch_scale=SCALAR[1]), int(np.rint(SCALAR[0] * L))),
                contour=(dict(time_scale=rho_c, pitch_scale=beta_c), contour_time_map(rho_c, beta_c, step, L)["L_out"]))
    out = {}
    for phase in ("independent", "shape"):
        for name, (kw, L_out) in maps.items():
            key = "synth_%s_%s" % (phase, name)
            out[key] = amd.eaQHMSynthesis(det, FS, L, phase=phase, **kw)
            out[key + RANGES] = amd.eaQHMSynthesis(det, FS, L, phase=phase, _ranges=split(L_out, 64, step), **kw)
    out["synth_shape_scalar_f0"] = amd.eaQHMSynthesis(det, FS, L, phase="shape", f0=amd.model_f0(det, FS) * 0.9,
                                                     **maps["scalar"][0])
    H = nz["hop"]
    for rho in (0.5, 2.0):
        L_out = int(np.rint(rho * L))
        tau = noise_time_map(H, L_out, rho)
        fund = amd.noise_fundamental(det, FS, tau, time_scale=rho, pitch_scale=SCALAR[1])
        for label, f in (("plain", None), ("mod", fund)):
            key = "noise_%s_rho%g" % (label, rho)
            out[key] = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=11, fundamental=f)
            out[key + RANGES] = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=11, fundamental=f,
                                                        _ranges=split(L_out, H))
    for phase, name in (("shape", "scalar"), ("independent", "contour")):
        kw = maps[name][0]
        out["synth_noise_%s_%s" % (phase, name)] = amd.eaQHMSynthesis(det, FS, L, phase=phase, noise=nz, noise_seed=11,
                                                                      **kw)
        out["synth_noise_mod_formant_%s_%s" % (phase, name)] = amd.eaQHMSynthesis(
            det, FS, L, phase=phase, noise=nz, noise_seed=11, noise_modulation=True, noise_formant=True,
            formant_scale=1.2, **kw)
    return out


def main(argv):
    sys.path.insert(0, os.path.dirname(HERE))
    import eaqhm_amd
    inp = inputs(eaqhm_amd)
    det, L = inp[:2]
    got = cases(eaqhm_amd, inp)
    doc = dict(parent_commit=argv[1], model="tests/golden/sa19_female_default.npz (reference_model()), residual of "
               "tests/golden/SA19.WAV", digest="sha256 of the C-contiguous float64 bytes", fs=FS, length=L,
               No_ti=len(det["ti"]), cases={k: digest(v) for k, v in got.items()})
    path = argv[2] if len(argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(got), path))
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
