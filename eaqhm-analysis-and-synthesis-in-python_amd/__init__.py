"""MI355X-native eaQHM analysis hot path (drop-in for the reference's functions.py entry points).

The package directory is named `eaqhm-analysis-and-synthesis-in-python_amd` (not importable by that
name); `import eaqhm_amd` at the repository root loads it under the module name `eaqhm_amd`.
"""
from .functions import (eaQHMAnalysisAndSynthesis, eaQHMAnalysisAndSynthesisBatch, eaqhmLS_complexamps,  # noqa: F401
                        iqhmLS_complexamps, phase_integr_interpolation)
from .hip import HipUnavailable, load_library  # noqa: F401
from .structs import Deterministic, Frame  # noqa: F401
from .model import (SCALE_RANGE, cepstrum_phase, model_from_parameters, model_parameters, alignment_index, alignment_time_scale, cepstrum_envelope, dtw, model_align, warp_rows, contour_time_map, eaQHMNoiseAnalysis, eaQHMNoiseModulation,  # noqa: F401
                    eaQHMNoiseSynthesis, eaQHMNoiseWarp, eaQHMSynthesis, formant_warp_vtln, model_cepstrum, model_envelope, model_f0,
                    model_phase, noise_alignment_index, noise_cepstrum, noise_envelope, noise_formant_contour, noise_formant_warp, noise_from_cepstrum, noise_fundamental, noise_time_map, noise_time_map_contour,
                    scale_contour, unpack_model, allpass_warp, cepstrum_rewarp, cepstrum_warp, check_cepstrum_warp,
                    rewarp_matrix)
from .convert import (check_conversion, check_conversion_arguments, check_gmm_arguments, check_gv_arguments,  # noqa: F401
                      check_kmeans_arguments, kmeans, kmeans_assign,
                      conversion_apply, conversion_pairs, conversion_train, conversion_trajectory, dynamic_rows,
                      f0_statistics, global_variance, gmm_fit, gmm_posteriors, gv_statistics, pitch_conversion_contour)
from .prologue import read_signal  # noqa: F401
