"""`python -m oatomobile_amd.baselines.torch.cil.train`: CIL training from datum files."""
