"""Linear ROMPC baseline (sofacontrol/baselines/rompc): Luenberger observer and resident control step (csrc/rompc.hip)."""
