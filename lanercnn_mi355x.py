"""Top-level plugin module so the reference's drivers can load the fork model of this build by name:
    python train_lanercnn.py -m lanercnn_mi355x      (import_module(args.model).get_model())"""
import lanegcn_amd  # noqa: F401  (import shim for the lanegcn-1_amd/ package directory)
from lanegcn_amd.lanercnn import *  # noqa: F401,F403
from lanegcn_amd.lanercnn import config, get_model, get_model_for_torch_dist  # noqa: F401
