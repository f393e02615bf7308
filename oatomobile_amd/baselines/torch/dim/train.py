"""Trains the deep imitative model on expert demonstrations (oatomobile/baselines/torch/dim/train.py):

    python -m oatomobile_amd.baselines.torch.dim.train --dataset_dir D --output_dir O --num_epochs N

See oatomobile_amd/baselines/torch/_train_main.py for the flags and outputs."""
import sys

from oatomobile_amd.baselines.torch._train_main import main

if __name__ == "__main__":
  sys.exit(main("dim"))
