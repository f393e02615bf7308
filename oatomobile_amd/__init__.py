"""oatomobile_amd — MI355X-native deep-imitative-model inference path of OATML/oatomobile.

Public surface mirrors `oatomobile.baselines.torch` (baselines/torch/__init__.py:17-21) for the
path in scope: `ImitativeModel`, `RIPAgent`, `DIMAgent`.
"""

from oatomobile_amd.agents import DIMAgent
from oatomobile_amd.agents import PlanStats
from oatomobile_amd.agents import RIPAgent
from oatomobile_amd.agents import SetPointAgent
from oatomobile_amd.model import ImitativeModel
from oatomobile_amd.model import transform_visual

from oatomobile_amd.cil import BehaviouralModel
from oatomobile_amd.cil import CILAgent
from oatomobile_amd.detection import detection_auroc
from oatomobile_amd.lidar import lidar_to_bev
from oatomobile_amd.prediction import Prediction
from oatomobile_amd.prediction import displacement_errors
from oatomobile_amd.prediction import min_over_k
from oatomobile_amd.prediction import philox_normal
from oatomobile_amd.train import CILTrainer
from oatomobile_amd.train import DIMTrainer

__all__ = ["ImitativeModel", "RIPAgent", "DIMAgent", "SetPointAgent", "transform_visual", "lidar_to_bev",
           "BehaviouralModel", "CILAgent", "DIMTrainer", "CILTrainer", "PlanStats", "detection_auroc", "Prediction",
           "philox_normal", "displacement_errors", "min_over_k"]
