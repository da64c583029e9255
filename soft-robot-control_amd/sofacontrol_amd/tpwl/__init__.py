from .sysid import (TPWLFitResult, TPWLHorizonError, TPWLPointSelection, TPWLSysID, fit_tpwl, horizon_error, horizon_plan,  # noqa: F401
                    one_step_error, points_by_distance, points_from_records)
