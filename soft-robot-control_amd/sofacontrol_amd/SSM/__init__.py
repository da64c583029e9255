from .sysid import SSMHorizonError, horizon_error, horizon_plan  # noqa: F401
