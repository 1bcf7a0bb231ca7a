"""SysID student distillation (the reference's stage 2: scripts/dagger_usv_sysid_loopz.py) on csrc/usv_sysid.hip."""
from .dagger import SysIDStudent, USVSysIDAgent, USVSysIDTrainer, action_head_mirror, load_teacher, metrics_dict, step_lr
from .history import HistoryStream
from .module import EncoderNN, StateHistoryEncoder, action_head_nn
from .vecenv import USVSysIDVecEnv

__all__ = ["SysIDStudent", "USVSysIDAgent", "USVSysIDTrainer", "action_head_mirror", "load_teacher", "metrics_dict", "step_lr",
           "HistoryStream", "EncoderNN", "StateHistoryEncoder", "action_head_nn", "USVSysIDVecEnv"]
