"""of_dis_amd -- MI355X-native (gfx950 HIP) DIS optical flow / stereo depth hot path.

Drop-in for lordnn/OF_DIS's OFClass / run_dense pipeline.  The compute lives in libofdis.so
(hand-written HIP kernels + C-ABI, include/ofdis.h); this package is a thin host-side mirror.
"""
from ._lib import (FE_BINS, FE_COUNT, FE_FL, FE_GT1, FE_GT3, FE_GT5, FE_LANES, FE_MAX, FE_NONFINITE, FE_NSTATS,  # noqa: F401
                   FE_S0_COUNT, FE_S0_SUM, FE_S1_COUNT, FE_S1_SUM, FE_S2_COUNT, FE_S2_SUM, FE_SUM)
from ._lib import (FIT_LANES, FIT_MAX_SAMPLES, IMG_F32, IMG_U8, INTERP_MAX_T, MM_NSTATS, MODE_DE, MODE_OF, MOTION_SIMILARITY,  # noqa: F401
                   MOTION_TRANSLATION, TRACK_LAST, FlowView, OfdisError, OutFormat, Params, build, lib, out_format)
from .ofclass import (Context, OFClass, algorithmic_bytes, auto_first_scale, error_percentile, error_summary,  # noqa: F401
                      fit_lattice, kernel_names, kernel_names_all, kernel_names_ext, motion_summary,
                      max_frames_per_launch, oppoint, out_geometry, params_from_strings, pixel_grid, read_flo, read_image, synth_pair, synth_shift_pair,
                      tfilter_radius_bytes, validate,
                      write_flo, write_pfm, write_pnm)

__version__ = "0.1.0"
