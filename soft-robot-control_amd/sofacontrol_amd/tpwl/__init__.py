from .sysid import (TPWLFitResult, TPWLPointSelection, TPWLSysID, fit_tpwl, one_step_error, points_by_distance,  # noqa: F401
                    points_from_records)
