"""egoego_release_amd — MI355X-native stage-2 motion-diffusion sampling for EgoEgo.

Only the sampling hot path lives here: HIP kernels + C ABI in csrc/, the Python
mirror of the reference's CondGaussianDiffusion interface in model.py.
"""
from .synthetic import ModelConfig, make_weights, make_head_windows, head_condition_mask  # noqa: F401
from .synthetic import Stage1Config, make_stage1_weights, make_stage1_train_batch  # noqa: F401
from .synthetic import make_flow_cnn_weights, make_flows  # noqa: F401
from .synthetic import make_body_model, make_body_poses  # noqa: F401
from .synthetic import make_eval_motion  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not need torch.cuda or the .so
    if name in ("CondGaussianDiffusion", "TransformerDiffusionModel"):
        from . import model
        return getattr(model, name)
    if name in ("HeadFormer", "HeadNormalFormer", "estimate_head_pose", "FlowFeatureExtractor", "split_headnet_state_dict"):
        from . import stage1
        return getattr(stage1, name)
    if name in ("BodyModel", "BodyEngine", "run_smpl_model", "save_verts_faces_to_mesh_file"):
        from . import body
        return getattr(body, name)
    if name in ("evaluate_samples", "determine_floor_height_and_contacts", "compute_metrics_for_smpl"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("build_motion_windows", "window_table", "MotionWindows", "MotionWindowDataset", "rest_pose_offsets"):
        from . import motion_data
        return getattr(motion_data, name)
    if name == "HipEngine":
        from .engine import HipEngine
        return HipEngine
    raise AttributeError(name)
