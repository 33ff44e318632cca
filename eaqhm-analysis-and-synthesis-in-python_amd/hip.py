"""ctypes binding of libeaqhm_hip.so (C ABI: include/eaqhm_hip.h).

There is NO CPU fallback: if the library is missing or no MI355X is visible, every entry point of
the package raises `HipUnavailable`.  Device buffers are torch-ROCm tensors; only their raw
`data_ptr()` crosses the ABI.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EAQHM_LIB: A/B measurements with an alternative build of the same library (tools/); the product default is in-tree
LIB_PATH = os.environ.get("EAQHM_LIB") or os.path.join(_HERE, "csrc", "libeaqhm_hip.so")

# every symbol include/eaqhm_hip.h itself declares: (name, restype, argtypes)
_P = C.c_void_p
_I32, _I64, _F64 = C.c_int32, C.c_int64, C.c_double
# EAQHM_ABI_VERSION (csrc/eaqhm_common.h) this binding was written for: argument lists change under unchanged names
ABI_VERSION = 6
# keys of eaqhm_set_option (EAQHM_OPT_* of the header)
OPT_LS_VARIANT, OPT_DEBUG_KEEP, OPT_DTW_PHASES, OPT_A0_RESIDENT = 1, 2, 3, 4
SYMBOLS = (
    ("eaqhm_ctx_create", C.c_int, [C.POINTER(_P), C.c_int]),
    ("eaqhm_ctx_destroy", C.c_int, [_P]),
    ("eaqhm_set_stream", C.c_int, [_P, _P]),
    ("eaqhm_sync", C.c_int, [_P]),
    ("eaqhm_last_error", C.c_char_p, [_P]),
    ("eaqhm_set_option", C.c_int, [_P, _I32, _I32]),
    ("eaqhm_debug_read", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("eaqhm_device_info", C.c_int, [_P, C.POINTER(_I32)]),
    ("eaqhm_ls_faults", C.c_int, [_P, C.POINTER(_I32)]),
    ("eaqhm_frame_prep", C.c_int, [_P, _P, _I64, _I64, _I64, _I32, _P, _I32, _P, _P, _P, _P]),
    ("eaqhm_ls_batch", C.c_int, [_P, _I32, _P, _I64, _F64, _P, _P, _I64, _I64, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                  _I32, _I32, _I32, _F64, _F64, _P, _P, _P]),
    ("eaqhm_ls_explicit", C.c_int, [_P, _P, _I32, _P, _P, _P, _I32, _P, _F64, _P, _P]),
    ("eaqhm_phase_integrate", C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P]),
    ("eaqhm_spline_solve", C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    ("eaqhm_spline_solve_range", C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    ("eaqhm_eval_synth", C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _F64, _I64, _I64, _I64, _I64, _I64, _P, _F64,
                                    _P, _P, _I64, _I64, _P, _P, _P, _P]),
    ("eaqhm_eval_partials_len", _I64, [_I64, _I64, _I32]),
    ("eaqhm_modify_prep", C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _F64, _P, _P, _P, _I32, _P, _P, _P]),
    ("eaqhm_modify_synth", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _F64, _F64, _F64, _I64, _I64, _I64,
                                      _P, _P, _P, _P, _F64, _P, _P]),
    ("eaqhm_model_envelope", C.c_int, [_P, _P, _I32, _I32, _P, _P, _I32, _P]),
    ("eaqhm_noise_analyse", C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P]),
    ("eaqhm_noise_synth", C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _I32, C.c_uint64, _I64, _I64, _I64, _P, _I32,
                                     _P, _I32, _P, _P]),
    ("eaqhm_noise_warp", C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P]),
    ("eaqhm_noise_envelope", C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _I32, _P]),
    ("eaqhm_noise_modulation", C.c_int, [_P, _P, _I64, _I32, _P, _P, _P, _I32, _F64, _F64, _F64, _I32, _P]),
    ("eaqhm_modify_amp_warp", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _P, _I32, _P]),
    ("eaqhm_model_envelope_warp", C.c_int, [_P, _P, _I32, _I32, _P, _P, _I32, _P, _I32, _P]),
    ("eaqhm_noise_warp_map", C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _I32, _P, _P]),
    ("eaqhm_noise_envelope_map", C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _I32, _P, _I32, _P]),
    ("eaqhm_model_cepstrum", C.c_int, [_P, _P, _I32, _I32, _F64, _I32, _F64, _P]),
    ("eaqhm_modify_amp_cepstrum", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _I32, _P, _P, _P, _I32, _P]),
    ("eaqhm_cepstrum_envelope", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _P, _I32, _P, _I32, _P]),
    ("eaqhm_cepstrum_cost", C.c_int, [_P, _P, _I32, _P, _I32, _I32, _F64, _F64, _I32, _P]),
    ("eaqhm_dtw", C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    ("eaqhm_model_build", C.c_int, [_P, _P, _P, _P, _P, _I32, _P, _I32, _F64, _I32, _I32, _I32, _P]),
    ("eaqhm_cepstrum_phase", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _P, _I32, _P, _I32, _P]),
    ("eaqhm_noise_cepstrum", C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P]),
    ("eaqhm_noise_from_cepstrum", C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    ("eaqhm_gmm_work_len", _I64, [_I64, _I32, _I32]),
    ("eaqhm_gmm_estep", C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    ("eaqhm_gmm_mstep", C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _P, _P]),
    ("eaqhm_gmm_regress", C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _P]),
)
# every symbol include/eaqhm_mlpg.h declares: a table of its own, bound with SYMBOLS
SYMBOLS_MLPG = (
    ("eaqhm_ceps_delta", C.c_int, [_P, _P, _I64, _I32, _I32, _P]),
    ("eaqhm_mlpg_work_len", _I64, [_I64, _I32, _I32]),
    ("eaqhm_mlpg_solve", C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _I64, _P, _P]),
)
# every symbol include/eaqhm_gv.h declares: likewise
SYMBOLS_GV = (
    ("eaqhm_gv_chunk_rows", _I64, [_I64]),
    ("eaqhm_gv_work_len", _I64, [_I64, _I32, _I32]),
    ("eaqhm_gv_ascend", C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _I64, _P, _P, _I32, _P, _P, _P]),
)
# every symbol include/eaqhm_cepwarp.h declares: each is its sibling's list plus one double, cep_warp
SYMBOLS_CEPWARP = (
    ("eaqhm_model_cepstrum_warped", C.c_int, [_P, _P, _I32, _I32, _F64, _I32, _F64, _P, _F64]),
    ("eaqhm_modify_amp_cepstrum_warped", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _I32, _P, _P, _P, _I32, _P, _F64]),
    ("eaqhm_cepstrum_envelope_warped", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _P, _I32, _P, _I32, _P, _F64]),
    ("eaqhm_cepstrum_phase_warped", C.c_int, [_P, _P, _I32, _I32, _F64, _P, _P, _P, _I32, _P, _I32, _P, _F64]),
    ("eaqhm_model_build_warped", C.c_int, [_P, _P, _P, _P, _P, _I32, _P, _I32, _F64, _I32, _I32, _I32, _P, _F64]),
    ("eaqhm_noise_from_cepstrum_warped", C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _F64]),
)
# every symbol include/eaqhm_kmeans.h declares: likewise
SYMBOLS_KMEANS = (
    ("eaqhm_kmeans_work_len", _I64, [_I64, _I32, _I32]),
    ("eaqhm_kmeans_assign", C.c_int, [_P, _P, _I64, _I64, _I32, _P, _P, _I32, _P, _P]),
    ("eaqhm_kmeans_update", C.c_int, [_P, _P, _I64, _I64, _I32, _P, _I32, _P, _P, _P, _P]),
)
# every symbol include/eaqhm_mlpg_em.h declares: likewise
SYMBOLS_MLPG_EM = (
    ("eaqhm_mlpg_estep", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _P, _P, _I64, _P, _P]),
)
# every symbol include/eaqhm_nn.h declares: likewise
SYMBOLS_NN = (
    ("eaqhm_nn_splits", _I32, [_I64, _I64]),
    ("eaqhm_nn_work_len", _I64, [_I64, _I64, _I32]),
    ("eaqhm_nn_rows", C.c_int, [_P, _P, _I64, _I64, _P, _I64, _I64, _I32, _P, _P, _P]),
)
# every symbol include/eaqhm_swipe.h declares: likewise
SYMBOLS_SWIPE = (
    ("eaqhm_swipe_loudness", C.c_int, [_P, _P, _I64, _I32, _I32, _I64, _I64, _P, _F64, _F64, _P, _P, _P, _I32, _P, _I64]),
    ("eaqhm_swipe_scores", C.c_int, [_P, _P, _I32, _I64, _P, _I64, _I64, _I32, _P]),
    ("eaqhm_swipe_pick", C.c_int, [_P, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _F64, _P, _P, _P, _P, _I32, _P, _P,
                                    _P]),
)
# every symbol include/eaqhm_viterbi.h declares: likewise
SYMBOLS_VITERBI = (
    ("eaqhm_viterbi_forward", C.c_int, [_P, _P, _I32, _I64, _P, _I32, _I32, _F64, _F64, _P, _P, _P]),
    ("eaqhm_viterbi_backtrack", C.c_int, [_P, _P, _P, _P, _I32, _I64, _P]),
    ("eaqhm_viterbi_refine", C.c_int, [_P, _P, _P, _I32, _I64, _P, _P, _P, _P, _P, _I32, _P, _P]),
)
# every symbol include/eaqhm_formant.h declares: likewise
SYMBOLS_FORMANT = (
    ("eaqhm_allpole_roots", C.c_int, [_P, _P, _I64, _I32, _P, _P]),
    ("eaqhm_formant_candidates", C.c_int, [_P, _P, _P, _I64, _I32, _F64, _F64, _F64, _F64, _P, _P, _P]),
    ("eaqhm_formant_forward", C.c_int, [_P, _P, _P, _P, _P, _I32, _I64, _F64, _F64, _P, _P]),
    ("eaqhm_formant_backtrack", C.c_int, [_P, _P, _P, _I32, _I64, _P, _P]),
)
# every symbol include/eaqhm_onset.h declares: likewise
SYMBOLS_ONSET = (
    ("eaqhm_onset_bands", C.c_int, [_P, _P, _I64, _I32, _I32, _I64, _P, _F64, _P, _I32, _F64, _P, _I64]),
    ("eaqhm_onset_flux", C.c_int, [_P, _P, _I64, _I64, _I32, _I32, _I64, _I64, _P]),
    ("eaqhm_onset_peaks", C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _F64, _P]),
)


class HipUnavailable(RuntimeError):
    """The HIP library or the GPU is missing.  The package has no CPU path."""


_lib = None


def load_library():
    """Load libeaqhm_hip.so and bind every symbol of the header (no GPU needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipUnavailable(
            "libeaqhm_hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This package has no CPU fallback." % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise HipUnavailable("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, res, args in (SYMBOLS + SYMBOLS_MLPG + SYMBOLS_GV + SYMBOLS_CEPWARP + SYMBOLS_KMEANS + SYMBOLS_MLPG_EM
                            + SYMBOLS_NN + SYMBOLS_SWIPE + SYMBOLS_VITERBI + SYMBOLS_FORMANT + SYMBOLS_ONSET):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipUnavailable("libeaqhm_hip.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(t):
    """Raw device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("device buffers must be contiguous GPU tensors")
    return t.data_ptr()


class Context:
    """One eaqhm_ctx bound to a device and to torch's current stream on it."""

    def __init__(self, device_index=0):
        import torch
        if not torch.cuda.is_available():
            raise HipUnavailable("no ROCm GPU visible (torch.cuda.is_available() is False); "
                                 "this package has no CPU fallback")
        self.lib = load_library()
        self.torch = torch
        self.device = torch.device("cuda", device_index)
        h = _P()
        rc = self.lib.eaqhm_ctx_create(C.byref(h), device_index)
        if rc != 0:
            raise HipUnavailable("eaqhm_ctx_create failed with code %d" % rc)
        self.h = h
        info = (_I32 * 4)()
        self._ck(self.lib.eaqhm_device_info(self.h, info))
        self.n_cu, self.lds_bytes, self.clock_khz, self.abi_version = [int(v) for v in info]
        if self.abi_version != ABI_VERSION:
            self.close()
            raise HipUnavailable("%s has ABI version %d, this binding needs %d: stale build, rebuild"
                                 % (LIB_PATH, self.abi_version, ABI_VERSION))
        v = os.environ.get("EAQHM_LS_VARIANT")          # A/B knobs for measurements (include/eaqhm_hip.h)
        if v:
            self.set_option(OPT_LS_VARIANT, int(v))
        v = os.environ.get("EAQHM_A0_RESIDENT")
        if v:
            self.set_option(OPT_A0_RESIDENT, int(v))
        self.bind_stream()

    def bind_stream(self):
        s = self.torch.cuda.current_stream(self.device)
        self._ck(self.lib.eaqhm_set_stream(self.h, _P(s.cuda_stream)))

    def _ck(self, rc):
        if rc != 0:
            msg = self.lib.eaqhm_last_error(self.h)
            raise RuntimeError("libeaqhm_hip error %d: %s" % (rc, msg.decode() if msg else "?"))

    def close(self):
        if getattr(self, "h", None):
            self.lib.eaqhm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._ck(self.lib.eaqhm_set_option(self.h, key, value))

    def debug_read(self):
        out = (C.c_uint64 * 16)()
        self._ck(self.lib.eaqhm_debug_read(self.h, out))
        return [int(v) for v in out]

    def ls_faults(self):
        """(LS systems whose Cholesky broke down, stalled diagonal pipelines, frames dropped because their window was not
        resident) since the last read (waits for the stream, clears the counts)."""
        n = (_I32 * 3)()
        self._ck(self.lib.eaqhm_ls_faults(self.h, n))
        return int(n[0]), int(n[1]), int(n[2])

    def sync(self):
        self._ck(self.lib.eaqhm_sync(self.h))

    # ---- thin wrappers (argument order = header order)
    def frame_prep(self, fm_cur, L, track_t0, track_len, Kmax, frame_c, n_frames, ncol, cols, seeded, any_seed):
        self._ck(self.lib.eaqhm_frame_prep(self.h, _ptr(fm_cur), L, track_t0, track_len, Kmax, _ptr(frame_c), n_frames,
                                           _ptr(ncol), _ptr(cols), _ptr(seeded), _ptr(any_seed)))

    def ls_batch(self, mode, s, L, fs, am_cur, fm_cur, track_t0, track_len, Kmax, frame_inst, frame_c, frame_wl,
                 frame_f0, frame_K, ncol, cols, seeded, any_seed, n_frames, wl_max, a_iter, f0_stale, f0min, records,
                 raw_amp=None, raw_slope=None):
        self._ck(self.lib.eaqhm_ls_batch(self.h, mode, _ptr(s), L, float(fs), _ptr(am_cur), _ptr(fm_cur), track_t0,
                                         track_len, Kmax,
                                         _ptr(frame_inst), _ptr(frame_c), _ptr(frame_wl), _ptr(frame_f0),
                                         _ptr(frame_K), _ptr(ncol), _ptr(cols), _ptr(seeded), _ptr(any_seed),
                                         n_frames, wl_max, a_iter, float(f0_stale), float(f0min),
                                         _ptr(records), _ptr(raw_amp), _ptr(raw_slope)))

    def ls_explicit(self, s, N, am, fm, f0range, Kc, window, fs, out_amp, out_slope):
        self._ck(self.lib.eaqhm_ls_explicit(self.h, _ptr(s), N, _ptr(am), _ptr(fm), _ptr(f0range), Kc, _ptr(window),
                                            float(fs), _ptr(out_amp), _ptr(out_slope)))

    def phase_integrate(self, omega, ph, knots, n_knots, first, last, out):
        self._ck(self.lib.eaqhm_phase_integrate(self.h, _ptr(omega), _ptr(ph), _ptr(knots), n_knots, first, last, _ptr(out)))

    def spline_solve(self, records, No_ti, Kmax, step, code, mom, i_lo=0, i_hi=None):
        i_hi = No_ti if i_hi is None else i_hi
        self._ck(self.lib.eaqhm_spline_solve_range(self.h, _ptr(records), No_ti, Kmax, step, i_lo, i_hi, _ptr(code),
                                                   _ptr(mom)))

    def eval_synth(self, records, code, mom, No_ti, Kmax, step, fs, L, t_lo, t_hi, s_lo, s_hi, target, std_det,
                   am_out, fm_out, track_t0, track_len, ph_knot, s_hat, partials, sums_out):
        self._ck(self.lib.eaqhm_eval_synth(self.h, _ptr(records), _ptr(code), _ptr(mom), No_ti, Kmax,
                                           step, float(fs), L, t_lo, t_hi, s_lo, s_hi, _ptr(target), float(std_det),
                                           _ptr(am_out), _ptr(fm_out), track_t0, track_len, _ptr(ph_knot), _ptr(s_hat),
                                           _ptr(partials), _ptr(sums_out)))

    def modify_prep(self, records, code, mom, No_ti, Kmax, step, fs, beta, gain, alpha, preserve_envelope, amp, R,
                    ph0):
        self._ck(self.lib.eaqhm_modify_prep(self.h, _ptr(records), _ptr(code), _ptr(mom), No_ti, Kmax, step, float(fs),
                                            _ptr(beta), _ptr(gain), _ptr(alpha), int(bool(preserve_envelope)),
                                            _ptr(amp), _ptr(R), _ptr(ph0)))

    def modify_synth(self, records, code, mom, amp, R, ph0, No_ti, Kmax, step, fs, rho, beta, L_out, t_lo, t_hi, out,
                     curve=None, shape=None):
        """curve = (C, rate, gain, rate_min): the contour map (rho, beta not read); shape = (f0, S): the shape phase."""
        C_, rate, gain, rate_min = curve or (None, None, None, 0.0)
        f0, S = shape or (None, None)
        self._ck(self.lib.eaqhm_modify_synth(self.h, _ptr(records), _ptr(code), _ptr(mom), _ptr(amp), _ptr(R), _ptr(ph0),
                                             No_ti, Kmax, step, float(fs), float(rho), float(beta), L_out, t_lo, t_hi,
                                             _ptr(out), _ptr(C_), _ptr(rate), _ptr(gain), float(rate_min), _ptr(f0),
                                             _ptr(S)))

    def model_envelope(self, records, No_ti, Kmax, alpha, freqs, F, out):
        self._ck(self.lib.eaqhm_model_envelope(self.h, _ptr(records), No_ti, Kmax, _ptr(alpha), _ptr(freqs), F,
                                               _ptr(out)))

    def noise_analyse(self, e, L, hop, order, sigma, refl):
        self._ck(self.lib.eaqhm_noise_analyse(self.h, _ptr(e), L, hop, order, _ptr(sigma), _ptr(refl)))

    def noise_synth(self, sigma, refl, Nf, hop, order, tau, Nq, seed, L_out, t_lo, t_hi, out, accumulate=False,
                    mod=None):
        """mod = (mod, harmonics, theta, nu): the pitch-synchronous modulation."""
        mod_, harmonics, theta, nu = mod or (None, 0, None, None)
        self._ck(self.lib.eaqhm_noise_synth(self.h, _ptr(sigma), _ptr(refl), Nf, hop, order, _ptr(tau), Nq, seed, L_out,
                                            t_lo, t_hi, _ptr(out), int(bool(accumulate)), _ptr(mod_), harmonics,
                                            _ptr(theta), _ptr(nu)))

    def noise_warp(self, sigma, refl, Nf, order, alpha, sigma_out, refl_out):
        self._ck(self.lib.eaqhm_noise_warp(self.h, _ptr(sigma), _ptr(refl), Nf, order, _ptr(alpha), _ptr(sigma_out),
                                           _ptr(refl_out)))

    def noise_envelope(self, sigma, refl, Nf, order, alpha, fnorm, F, out):
        self._ck(self.lib.eaqhm_noise_envelope(self.h, _ptr(sigma), _ptr(refl), Nf, order, _ptr(alpha), _ptr(fnorm), F,
                                               _ptr(out)))

    def noise_modulation(self, e, L, hop, theta, f0, voiced, No_ti, ti0, step, fs, harmonics, mod):
        self._ck(self.lib.eaqhm_noise_modulation(self.h, _ptr(e), L, hop, _ptr(theta), _ptr(f0), _ptr(voiced), No_ti,
                                                 float(ti0), float(step), float(fs), harmonics, _ptr(mod)))

    # the piecewise-linear formant warp: f_in [B], f_out [rows][B] (Hz for the model, cycles per sample for the noise)
    def modify_amp_warp(self, records, No_ti, Kmax, fs, beta, f_in, f_out, B, amp):
        self._ck(self.lib.eaqhm_modify_amp_warp(self.h, _ptr(records), No_ti, Kmax, float(fs), _ptr(beta), _ptr(f_in),
                                                _ptr(f_out), B, _ptr(amp)))

    def model_envelope_warp(self, records, No_ti, Kmax, f_in, f_out, B, freqs, F, out):
        self._ck(self.lib.eaqhm_model_envelope_warp(self.h, _ptr(records), No_ti, Kmax, _ptr(f_in), _ptr(f_out), B,
                                                    _ptr(freqs), F, _ptr(out)))

    def noise_warp_map(self, sigma, refl, Nf, order, f_in, f_out, B, sigma_out, refl_out):
        self._ck(self.lib.eaqhm_noise_warp_map(self.h, _ptr(sigma), _ptr(refl), Nf, order, _ptr(f_in), _ptr(f_out), B,
                                               _ptr(sigma_out), _ptr(refl_out)))

    def noise_envelope_map(self, sigma, refl, Nf, order, f_in, f_out, B, fnorm, F, out):
        self._ck(self.lib.eaqhm_noise_envelope_map(self.h, _ptr(sigma), _ptr(refl), Nf, order, _ptr(f_in), _ptr(f_out),
                                                   B, _ptr(fnorm), F, _ptr(out)))

    # the discrete-cepstrum envelope: ceps [rows][order + 1]; warp = (f_in [B], f_out [rows][B], B) excludes alpha [rows]
    def model_cepstrum(self, records, No_ti, Kmax, fs, order, lam, ceps):
        self._ck(self.lib.eaqhm_model_cepstrum(self.h, _ptr(records), No_ti, Kmax, float(fs), order, float(lam),
                                               _ptr(ceps)))

    def modify_amp_cepstrum(self, records, No_ti, Kmax, fs, beta, ceps, order, amp, alpha=None, warp=None):
        f_in, f_out, B = warp or (None, None, 0)
        self._ck(self.lib.eaqhm_modify_amp_cepstrum(self.h, _ptr(records), No_ti, Kmax, float(fs), _ptr(beta),
                                                    _ptr(ceps), order, _ptr(alpha), _ptr(f_in), _ptr(f_out), B,
                                                    _ptr(amp)))

    def cepstrum_envelope(self, ceps, n, order, fs, freqs, F, out, alpha=None, warp=None):
        f_in, f_out, B = warp or (None, None, 0)
        self._ck(self.lib.eaqhm_cepstrum_envelope(self.h, _ptr(ceps), n, order, float(fs), _ptr(alpha), _ptr(f_in),
                                                  _ptr(f_out), B, _ptr(freqs), F, _ptr(out)))

    # the time alignment: band [nA][2 r + 1], cell (i, j) at [i][j - c_i + r] (include/eaqhm_hip.h)
    def cepstrum_cost(self, cepsA, nA, cepsB, nB, order, c0_weight, empty_cost, r, band_out):
        self._ck(self.lib.eaqhm_cepstrum_cost(self.h, _ptr(cepsA), nA, _ptr(cepsB), nB, order, float(c0_weight),
                                              float(empty_cost), r, _ptr(band_out)))

    def dtw(self, band, nA, nB, r, ptr, path, path_len, total):
        """band holds the costs on entry and D on return; path int32[nA + nB - 1, 2], path_len int32[1], total
        float64[1] are device tensors."""
        self._ck(self.lib.eaqhm_dtw(self.h, _ptr(band), nA, nB, r, _ptr(ptr), _ptr(path), _ptr(path_len), _ptr(total)))

    # a harmonic model from f0 and cepstral rows: voiced uint8[n], records [n][3 Kmax + 1]
    def model_build(self, f0, theta, voiced, ceps, order, a0, n, fs, Kmax, Kcap, zero_phase, records):
        self._ck(self.lib.eaqhm_model_build(self.h, _ptr(f0), _ptr(theta), _ptr(voiced), _ptr(ceps), order, _ptr(a0), n,
                                            float(fs), Kmax, Kcap, int(bool(zero_phase)), _ptr(records)))

    def cepstrum_phase(self, ceps, n, order, fs, freqs, F, out, alpha=None, warp=None):
        f_in, f_out, B = warp or (None, None, 0)
        self._ck(self.lib.eaqhm_cepstrum_phase(self.h, _ptr(ceps), n, order, float(fs), _ptr(alpha), _ptr(f_in),
                                               _ptr(f_out), B, _ptr(freqs), F, _ptr(out)))

    # the noise model to and from cepstral rows: ceps [Nf][Q + 1], refl [Nf][p]
    def noise_cepstrum(self, sigma, refl, Nf, p, Q, ceps):
        self._ck(self.lib.eaqhm_noise_cepstrum(self.h, _ptr(sigma), _ptr(refl), Nf, p, Q, _ptr(ceps)))

    def noise_from_cepstrum(self, ceps, Nf, Q, p, sigma_out, refl_out):
        self._ck(self.lib.eaqhm_noise_from_cepstrum(self.h, _ptr(ceps), Nf, Q, p, _ptr(sigma_out), _ptr(refl_out)))

    # the joint-density mixture of the spectral conversion: Z [N][D] centred rows, gamma [N][M]
    def gmm_work_len(self, N, D, M):
        return int(self.lib.eaqhm_gmm_work_len(N, D, M))

    def gmm_estep(self, Z, N, D, M, mu, W, k, gamma_out, ll_out):
        self._ck(self.lib.eaqhm_gmm_estep(self.h, _ptr(Z), N, D, M, _ptr(mu), _ptr(W), _ptr(k), _ptr(gamma_out),
                                          _ptr(ll_out)))

    def gmm_mstep(self, Z, gamma, N, D, M, work, S0, S1, S2):
        self._ck(self.lib.eaqhm_gmm_mstep(self.h, _ptr(Z), _ptr(gamma), N, D, M, _ptr(work), _ptr(S0), _ptr(S1),
                                          _ptr(S2)))

    def gmm_regress(self, X, gamma, A, b, N, dx, dy, M, Y_out):
        self._ck(self.lib.eaqhm_gmm_regress(self.h, _ptr(X), _ptr(gamma), _ptr(A), _ptr(b), N, dx, dy, M, _ptr(Y_out)))

    # delta rows and the trajectory solve: P, r [n][2 dy] static half first, runs int64 device tensors
    def ceps_delta(self, C_, n, cols, span, out):
        self._ck(self.lib.eaqhm_ceps_delta(self.h, _ptr(C_), n, cols, span, _ptr(out)))

    def mlpg_work_len(self, n, dy, span):
        return int(self.lib.eaqhm_mlpg_work_len(n, dy, span))

    def mlpg_solve(self, P, r, n, dy, span, run_start, run_len, n_runs, work, Y):
        self._ck(self.lib.eaqhm_mlpg_solve(self.h, _ptr(P), _ptr(r), n, dy, span, _ptr(run_start), _ptr(run_len), n_runs,
                                           _ptr(work), _ptr(Y)))

    # the global-variance ascent: Y holds y_ML on entry; trace a float64[iters + 1, dy] tensor or None
    def gv_chunk_rows(self, n):
        return int(self.lib.eaqhm_gv_chunk_rows(n))

    def gv_work_len(self, n, dy, span):
        return int(self.lib.eaqhm_gv_work_len(n, dy, span))

    def gv_ascend(self, P, r, n, dy, span, run_start, run_len, n_runs, gv_mean, gv_prec, iters, work, Y, trace=None):
        self._ck(self.lib.eaqhm_gv_ascend(self.h, _ptr(P), _ptr(r), n, dy, span, _ptr(run_start), _ptr(run_len), n_runs,
                                          _ptr(gv_mean), _ptr(gv_prec), iters, _ptr(work), _ptr(Y), _ptr(trace)))

    # the conditional E-step of the trajectory refinement: dy counts the static target columns, A
    # [M][2 dy][dx], bq and py [M][2 dy], Y [n][dy]; rows outside every run are not written
    def mlpg_estep(self, X, prior, A, bq, py, kc, Y, n, dx, dy, M, span, run_start, run_len, n_runs, gamma_out, ll_out):
        self._ck(self.lib.eaqhm_mlpg_estep(self.h, _ptr(X), _ptr(prior), _ptr(A), _ptr(bq), _ptr(py), _ptr(kc), _ptr(Y), n,
                                           dx, dy, M, span, _ptr(run_start), _ptr(run_len), n_runs, _ptr(gamma_out),
                                           _ptr(ll_out)))

    # the k-means codebook: Z [N][ldz] rows of which the first D columns count, labels int32 [N],
    # changed int32 [ceil(N / 64)], count int64 [K]
    def kmeans_work_len(self, N, D, K):
        return int(self.lib.eaqhm_kmeans_work_len(N, D, K))

    def kmeans_assign(self, Z, N, ldz, D, C_, g, K, labels, changed):
        self._ck(self.lib.eaqhm_kmeans_assign(self.h, _ptr(Z), N, ldz, D, _ptr(C_), _ptr(g), K, _ptr(labels),
                                              _ptr(changed)))

    def kmeans_update(self, Z, N, ldz, D, labels, K, work, count, S1, Q):
        self._ck(self.lib.eaqhm_kmeans_update(self.h, _ptr(Z), N, ldz, D, _ptr(labels), K, _ptr(work), _ptr(count),
                                              _ptr(S1), _ptr(Q)))

    # nearest rows: A [nA][lda], B [nB][ldb] rows of which the first D columns count, work float64
    # [nn_work_len], index int64 [nA], dist2 float64 [nA]
    def nn_splits(self, nA, nB):
        return int(self.lib.eaqhm_nn_splits(nA, nB))

    def nn_work_len(self, nA, nB, D):
        return int(self.lib.eaqhm_nn_work_len(nA, nB, D))

    def nn_rows(self, A, nA, lda, B, nB, ldb, D, work, index, dist2):
        self._ck(self.lib.eaqhm_nn_rows(self.h, _ptr(A), nA, lda, _ptr(B), nB, ldb, D, _ptr(work), _ptr(index),
                                        _ptr(dist2)))

    # SWIPE' (DESIGN.md §13): x [n], window [w], lo int32 [nE], xlo, df [nE], L [nframes][ld]; K [cand][ldk], Si
    # [cand][nframes]; the windows of a pick are a sequence of (Si, j0, ncand, nframes, mu, tshift), S is None or [npc][T]
    def swipe_loudness(self, x, n, w, hop, pad, nframes, window, fs, sumw2, lo, xlo, df, nE, L, ld):
        self._ck(self.lib.eaqhm_swipe_loudness(self.h, _ptr(x), n, w, hop, pad, nframes, _ptr(window), float(fs),
                                               float(sumw2), _ptr(lo), _ptr(xlo), _ptr(df), nE, _ptr(L), ld))

    def swipe_scores(self, K, cand, ldk, L, nframes, ldl, nE, Si):
        self._ck(self.lib.eaqhm_swipe_scores(self.h, _ptr(K), cand, ldk, _ptr(L), nframes, ldl, nE, _ptr(Si)))

    def swipe_pick(self, windows, t, T, npc, pc0, ntc, nftc, ptab, nf, nfmax, p, s, S=None):
        n = len(windows)
        ptrs = lambda k: (_P * n)(*[_ptr(w[k]) for w in windows])  # noqa: E731
        self._ck(self.lib.eaqhm_swipe_pick(self.h, n, ptrs(0), (_I32 * n)(*[w[1] for w in windows]),
                                           (_I32 * n)(*[w[2] for w in windows]), (_I64 * n)(*[w[3] for w in windows]),
                                           ptrs(4), ptrs(5), _ptr(t), T, npc, float(pc0), _ptr(ntc), _ptr(nftc),
                                           _ptr(ptab), _ptr(nf), nfmax, _ptr(p), _ptr(s), _ptr(S)))

    # the continuous pitch track: S [npc][T], cost [W + 1] on the device, bp int16 [T][npc + 1], tilemap
    # int16 [ceil(T / 8)][npc + 1], last [npc + 1], q int32 [T]; unvoiced is None or (uv, vcost)
    def viterbi_forward(self, S, npc, T, cost, W, unvoiced, bp, tilemap, last):
        uv, vcost = unvoiced or (0.0, 0.0)
        self._ck(self.lib.eaqhm_viterbi_forward(self.h, _ptr(S), npc, T, _ptr(cost), W, int(unvoiced is not None),
                                                float(uv), float(vcost), _ptr(bp), _ptr(tilemap), _ptr(last)))

    def viterbi_backtrack(self, bp, tilemap, last, npc, T, q):
        self._ck(self.lib.eaqhm_viterbi_backtrack(self.h, _ptr(bp), _ptr(tilemap), _ptr(last), npc, T, _ptr(q)))

    def viterbi_refine(self, S, q, npc, T, pc, ntc, nftc, ptab, nf, nfmax, p, s):
        self._ck(self.lib.eaqhm_viterbi_refine(self.h, _ptr(S), _ptr(q), npc, T, _ptr(pc), _ptr(ntc), _ptr(nftc),
                                               _ptr(ptab), _ptr(nf), nfmax, _ptr(p), _ptr(s)))

    # formant tracks: refl [Nf][p], roots [Nf][p][2], iters int32 [Nf]; cand_f, cand_b [Nf][8], count int32
    # [Nf]; L [T][N][8], lf [T][8], states int8 [S][N], bp int16 [T][S], last [S], q int32 [T], total [1]
    def allpole_roots(self, refl, Nf, p, roots, iters):
        self._ck(self.lib.eaqhm_allpole_roots(self.h, _ptr(refl), Nf, p, _ptr(roots), _ptr(iters)))

    def formant_candidates(self, roots, iters, Nf, p, fs, fmin, fmax, bw_max, cand_f, cand_b, count):
        self._ck(self.lib.eaqhm_formant_candidates(self.h, _ptr(roots), _ptr(iters), Nf, p, float(fs), float(fmin),
                                                   float(fmax), float(bw_max), _ptr(cand_f), _ptr(cand_b), _ptr(count)))

    def formant_forward(self, L, lf, count, states, N, T, w_jump, absent_cost, bp, last):
        self._ck(self.lib.eaqhm_formant_forward(self.h, _ptr(L), _ptr(lf), _ptr(count), _ptr(states), N, T,
                                                float(w_jump), float(absent_cost), _ptr(bp), _ptr(last)))

    def formant_backtrack(self, bp, last, N, T, q, total):
        self._ck(self.lib.eaqhm_formant_backtrack(self.h, _ptr(bp), _ptr(last), N, T, _ptr(q), _ptr(total)))

    # transient onsets: x [n], window [w], k a HOST sequence of B + 1 bin edges, L [nframes][ld]; d [nframes];
    # flag uint8 [nframes]
    def onset_bands(self, x, n, w, hop, nframes, window, inv_sumw2, k, B, floor, L, ld):
        self._ck(self.lib.eaqhm_onset_bands(self.h, _ptr(x), n, w, hop, nframes, _ptr(window), float(inv_sumw2),
                                            (_I32 * (B + 1))(*[int(v) for v in k]), B, float(floor), _ptr(L), ld))

    def onset_flux(self, L, nframes, ld, B, lag, whole_lo, whole_hi, d):
        self._ck(self.lib.eaqhm_onset_flux(self.h, _ptr(L), nframes, ld, B, lag, whole_lo, whole_hi, _ptr(d)))

    def onset_peaks(self, d, nframes, pre_max, post_max, pre_avg, post_avg, delta, flag):
        self._ck(self.lib.eaqhm_onset_peaks(self.h, _ptr(d), nframes, pre_max, post_max, pre_avg, post_avg, float(delta),
                                            _ptr(flag)))

    # the cepstrum on an all-pass warped axis: each is its sibling above plus cep_warp, |cep_warp| <= 0.9
    def model_cepstrum_warped(self, records, No_ti, Kmax, fs, order, lam, ceps, cep_warp):
        self._ck(self.lib.eaqhm_model_cepstrum_warped(self.h, _ptr(records), No_ti, Kmax, float(fs), order, float(lam),
                                                      _ptr(ceps), float(cep_warp)))

    def modify_amp_cepstrum_warped(self, records, No_ti, Kmax, fs, beta, ceps, order, amp, cep_warp, alpha=None,
                                   warp=None):
        f_in, f_out, B = warp or (None, None, 0)
        self._ck(self.lib.eaqhm_modify_amp_cepstrum_warped(self.h, _ptr(records), No_ti, Kmax, float(fs), _ptr(beta),
                                                           _ptr(ceps), order, _ptr(alpha), _ptr(f_in), _ptr(f_out), B,
                                                           _ptr(amp), float(cep_warp)))

    def cepstrum_envelope_warped(self, ceps, n, order, fs, freqs, F, out, cep_warp, alpha=None, warp=None):
        f_in, f_out, B = warp or (None, None, 0)
        self._ck(self.lib.eaqhm_cepstrum_envelope_warped(self.h, _ptr(ceps), n, order, float(fs), _ptr(alpha),
                                                         _ptr(f_in), _ptr(f_out), B, _ptr(freqs), F, _ptr(out),
                                                         float(cep_warp)))

    def cepstrum_phase_warped(self, ceps, n, order, fs, freqs, F, out, cep_warp, alpha=None, warp=None):
        f_in, f_out, B = warp or (None, None, 0)
        self._ck(self.lib.eaqhm_cepstrum_phase_warped(self.h, _ptr(ceps), n, order, float(fs), _ptr(alpha), _ptr(f_in),
                                                      _ptr(f_out), B, _ptr(freqs), F, _ptr(out), float(cep_warp)))

    def model_build_warped(self, f0, theta, voiced, ceps, order, a0, n, fs, Kmax, Kcap, zero_phase, records, cep_warp):
        self._ck(self.lib.eaqhm_model_build_warped(self.h, _ptr(f0), _ptr(theta), _ptr(voiced), _ptr(ceps), order,
                                                   _ptr(a0), n, float(fs), Kmax, Kcap, int(bool(zero_phase)),
                                                   _ptr(records), float(cep_warp)))

    def noise_from_cepstrum_warped(self, ceps, Nf, Q, p, sigma_out, refl_out, cep_warp):
        self._ck(self.lib.eaqhm_noise_from_cepstrum_warped(self.h, _ptr(ceps), Nf, Q, p, _ptr(sigma_out), _ptr(refl_out),
                                                           float(cep_warp)))

    def eval_partials_len(self, t_lo, t_hi, step):
        return int(self.lib.eaqhm_eval_partials_len(t_lo, t_hi, step))
