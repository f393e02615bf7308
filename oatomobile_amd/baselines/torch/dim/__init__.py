"""`python -m oatomobile_amd.baselines.torch.dim.train`: DIM training from datum files."""
