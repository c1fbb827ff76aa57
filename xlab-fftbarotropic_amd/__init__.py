"""MI355X-native hot path of XLab-FFTBarotropic: pseudospectral RK4 step behind a C ABI.

The directory name carries a hyphen (as the project name does); import it with
`importlib.import_module("xlab-fftbarotropic_amd")` or through the alias module
`xlab_fftbarotropic_amd` at the repository root.
"""
from .binding import FftBaroError, FftwfOperation, Model, lib, read_field, write_field, make_field, make_source_kuo2004, EXPORTS, EDDY_DIFFUSIVITY_COLUMNS, SPECTRA_COLUMNS, spectra_shells, AZIMUTHAL_COLUMNS, azimuthal_cols, TANGENT_NORMS, tangent_kind, lyapunov, singular_values, TANGENTS_MAX, lyapunov_spectrum, kaplan_yorke, PARTICLE_STRETCHING_COLUMNS, CENSUS_COLUMNS, CENSUS_SHAPE_COLUMNS, census_shapes, clv, clv_coefficients, ClvResult, OBS_KINDS, POSITION, Observations, fourdvar, fit_initial, ADJOINTS_MAX, singular_vectors, checkpoint_every, gauss_newton_hvp, fit_incremental  # noqa: F401
from .build import build_lib  # noqa: F401
