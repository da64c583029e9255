from .sysid import TPWLFitResult, TPWLSysID, fit_tpwl, one_step_error, points_from_records  # noqa: F401
