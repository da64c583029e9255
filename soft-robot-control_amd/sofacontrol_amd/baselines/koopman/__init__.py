"""Koopman MPC baseline (sofacontrol/baselines/koopman): device lift and resident MPC step (csrc/koopman.hip)."""
