"""ctypes binding of the C ABI in ``include/sgw.h`` (``sorrel_amd/csrc/libsgw.so``).

There is no CPU fallback: if the HIP library is missing, or a second HIP runtime
gets mapped next to PyTorch's, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

MAX_TYPES, MAX_CHANNELS, MAX_CHOICES, MAX_ACTIONS, MAX_AGENTS, MAX_LAYERS, MAX_DIM = 32, 16, 8, 16, 128, 7, 256
RULE_NONE, RULE_SPAWN, RULE_BECOME_IF = 0, 1, 2
NO_BORDER = 255
STEP_SWEEP, STEP_RANDOM_ACTIONS, STEP_NO_OBS, STEP_OBS_NEXT, STEP_OBS_NEXT_PACKED, STEP_NO_MOVE, STEP_OBS_AGENT_MAJOR = 1, 2, 4, 8, 16, 32, 64
OBS_POST_NONE, OBS_POST_CLIP255_DIV255 = 0, 1
AGENT_RULE_MOVE, AGENT_RULE_TAG, AGENT_RULE_CLEANUP = 0, 1, 2
ACTION_MOVE, ACTION_CLEAN, ACTION_ZAP = 0, 1, 2
OBS_F32, OBS_U8 = 0, 1
STATUS_OOB_MOVE, STATUS_BAD_ACTION, STATUS_BAD_TYPE, STATUS_BAD_POS = 1, 2, 4, 8
CAP_OBSERVE_ROWS, CAP_ACT, CAP_RESOLVE, CAP_OBS_AGENT_MAJOR, CAP_SWEEP_ROWS = 1, 2, 4, 8, 16
ACT_U8, ACT_I32, ACT_I64, ACT_QF32 = 0, 1, 2, 3
STREAM_VALUE = 8            # which of its two values a type with a drawn value is worth (index = target cell)
NO_TARGET = 255             # target_types: the agent's action was invalid or aimed outside the grid
NO_SLOT = 255               # sgw_bind_encounters: a type that is not counted
TAIL_NONE, TAIL_AGENT_IS_IT, TAIL_POSITION_TABLE = 0, 1, 2
OK, EINVAL, EHIP, ENOMEM = 0, -1, -2, -3
RENDER_COMPOSITE, RENDER_LAYERS = 0, 1
TILE_OPAQUE, TILE_CLEAR, TILE_KEEP = 1, 2, 0xFFFF
STREAM_SAMPLE = 9           # sgw_sample's drawn (start, env) pairs: epoch 0, turn / env slots = low / high word of the draw counter
SAMPLE_F32, SAMPLE_U8 = 0, 1
SAMPLE_ACT_I64, SAMPLE_ACT_U8 = 0, 1
RETURNS_NORM_NONE, RETURNS_NORM_COLUMN, RETURNS_NORM_ALL = 0, 1, 2
RETURNS_OUT_F64, RETURNS_OUT_F32 = 0, 1
STREAM_TAU = 11             # sgw_iqn_forward's taus: index = (agent << 4) | (quantile >> 2), word quantile & 3, turn = the turn in flight
STREAM_POLICY = 10          # sgw_policy_sample's draw: index = agent, turn = the turn in flight (STREAM_EXPLORE's layout)
POLICY_F32, POLICY_F64 = 0, 1
POLICY_PROBS, POLICY_LOGITS = 0, 1
POLICY_MAX_ACTIONS = 256
PPO_ACT_I64, PPO_ACT_U8 = 0, 1
IQN_MAX_QUANTILES = 64
IQN_STATE_F32, IQN_STATE_U8 = 0, 1
IQN_MAX_LAYER, IQN_MAX_ACTIONS, IQN_N_COS = 256, 64, 64      # of sgw_iqn_forward (sgw_iqn_loss takes POLICY_MAX_ACTIONS)
ADAM_CLIP_NONE, ADAM_CLIP_NORM, ADAM_CLIP_COEF = 0, 1, 2
ADAM_ZERO_GRADS = 1
ADAM_MAX_TENSORS, ADAM_CHUNK = 4096, 4096
STREAM_NOISE = 12            # sgw_noisy_weights' normals: index = element, turn / env slots = the draw counter's words, epoch slot = tensor_id
NOISY_MAX_JOBS = 24
NOISY_FORWARD, NOISY_BACKWARD = 0, 1
POLICY_INVALID_ACTION = 255  # the action of a row torch's Categorical would raise for (its log-probability and entropy are NaN)


class SgwConfig(C.Structure):
    """Mirror of ``struct sgw_config`` (include/sgw.h); tests/test_abi.py checks the layout of every mirror in this module."""

    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32), ("layers", C.c_int32),
        ("num_agents", C.c_int32), ("vision_radius", C.c_int32),
        ("num_types", C.c_int32), ("num_channels", C.c_int32), ("num_actions", C.c_int32),
        ("agent_layer", C.c_int32), ("default_type", C.c_int32), ("fill_type", C.c_int32),
        ("obs_post", C.c_int32),
        ("action_dy", C.c_int8 * MAX_ACTIONS), ("action_dx", C.c_int8 * MAX_ACTIONS),
        ("agent_type", C.c_uint8 * MAX_AGENTS),
        ("type_value", C.c_double * MAX_TYPES),
        ("type_passable", C.c_uint8 * MAX_TYPES),
        ("type_rule", C.c_uint8 * MAX_TYPES),
        ("spawn_prob", C.c_double * MAX_TYPES),
        ("spawn_count", C.c_uint8 * MAX_TYPES),
        ("spawn_choice", (C.c_uint8 * MAX_CHOICES) * MAX_TYPES),
        ("appearance", (C.c_double * MAX_CHANNELS) * MAX_TYPES),
        ("layer_fill_type", C.c_uint8 * 8),
        ("layer_border_type", C.c_uint8 * 8),
        ("dense_prob", C.c_double),
        ("dense_count", C.c_uint8),
        ("dense_choice", C.c_uint8 * MAX_CHOICES),
        ("agent_rule", C.c_uint8), ("tag_it_type", C.c_uint8), ("tag_notit_type", C.c_uint8),
        ("reserved1", C.c_uint8 * 4),
        ("seed", C.c_uint64),
        ("first_env_id", C.c_uint64),
        ("num_envs", C.c_int64),
        ("tag_reward", C.c_double),
        ("rule_layer", C.c_int8 * MAX_TYPES), ("rule_become", C.c_uint8 * MAX_TYPES), ("rule_mask", C.c_uint32 * MAX_TYPES),
        ("action_kind", C.c_uint8 * MAX_ACTIONS), ("beam_radius", C.c_int32),
        ("clean_beam_type", C.c_uint8), ("zap_beam_type", C.c_uint8), ("reserved2", C.c_uint8 * 2),
        ("beam_block_mask", C.c_uint32), ("reward_total_factor", C.c_int32),
        ("grid_env_stride", C.c_int64),
        # drawn values (0.3): a pure suffix
        ("type_value_alt", C.c_double * MAX_TYPES), ("value_alt_prob", C.c_double * MAX_TYPES),
    ]


FAMILY_WAVE, FAMILY_WORKGROUP, FAMILY_GENERIC = 1, 2, 3


class SgwPlan(C.Structure):
    """Mirror of ``struct sgw_plan_info`` (include/sgw.h): what ``sgw_create`` decides for a config, as pure host arithmetic."""

    _fields_ = [
        ("family", C.c_int32), ("lanes_per_env", C.c_int32), ("threads", C.c_int32), ("grid_blocks", C.c_int32),
        ("lds_bytes", C.c_int64),
        ("env_lds", C.c_int32), ("obs_stage", C.c_int32), ("stage_agents", C.c_int32), ("whole_env_burst", C.c_int32),
        ("big_stage", C.c_int32), ("big_pitch", C.c_int32),
        ("onehot", C.c_int32), ("rgb16", C.c_int32), ("rules", C.c_int32),
        ("specialised", C.c_int32), ("phase_kernel", C.c_int32), ("rollout_in_one_launch", C.c_int32),
        ("walk_blocks", C.c_int32),
        ("walk_min_envs", C.c_int64), ("walk_max_envs", C.c_int64), ("big_stage_min_envs", C.c_int64),
        ("kernel", C.c_char * 192), ("kernel_prebuilt", C.c_char * 192), ("kernel_plain", C.c_char * 192),
        ("kernel_rollout", C.c_char * 192), ("kernel_walk", C.c_char * 192),
        ("kernel_phase", C.c_char * 96), ("kernel_observe_rows", C.c_char * 96),
    ]

    def as_dict(self) -> dict:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = v.decode() if isinstance(v, bytes) else int(v)
        return out


class SgwTurnRows(C.Structure):
    """Mirror of ``struct sgw_turn_rows`` (include/sgw.h): the agents' replay rings for ``sgw_turn_bind``."""

    _fields_ = [
        ("states", C.c_void_p * MAX_AGENTS), ("rewards", C.c_void_p * MAX_AGENTS), ("actions", C.c_void_p * MAX_AGENTS),
        ("dones", C.c_void_p * MAX_AGENTS),
        ("capacity", C.c_int64 * MAX_AGENTS), ("row", C.c_int64 * MAX_AGENTS), ("step", C.c_int64 * MAX_AGENTS),
        ("row_elems", C.c_int64 * MAX_AGENTS),
    ]


class SgwRenderDesc(C.Structure):
    """Mirror of ``struct sgw_render_desc`` (include/sgw.h): one ``sgw_render`` call."""

    _fields_ = [
        ("grid", C.c_void_p), ("atlas", C.c_void_p), ("tile_flags", C.c_void_p), ("type_tile", C.c_void_p),
        ("agent_pos", C.c_void_p), ("agent_tile", C.c_void_p), ("env_ids", C.c_void_p), ("centres", C.c_void_p),
        ("out", C.c_void_p),
        ("num_envs", C.c_int64), ("n", C.c_int64), ("grid_env_stride", C.c_int64),
        ("layers", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("num_agents", C.c_int32), ("agent_layer", C.c_int32),
        ("n_tiles", C.c_int32), ("th", C.c_int32), ("tw", C.c_int32),
        ("k", C.c_int32), ("vision", C.c_int32), ("oob_tile", C.c_int32), ("mode", C.c_int32),
    ]


class SgwSampleDesc(C.Structure):
    """Mirror of ``struct sgw_sample_desc`` (include/sgw.h): one ``sgw_sample`` call."""

    _fields_ = [
        ("states", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
        ("starts", C.c_void_p), ("envs", C.c_void_p), ("draw_count", C.c_void_p),
        ("out_states", C.c_void_p), ("out_next_states", C.c_void_p), ("out_actions", C.c_void_p),
        ("out_rewards", C.c_void_p), ("out_dones", C.c_void_p), ("out_valid", C.c_void_p), ("out_index", C.c_void_p),
        ("n", C.c_int64), ("capacity", C.c_int64), ("num_envs", C.c_int64), ("num_starts", C.c_int64), ("row_elems", C.c_int64),
        ("state_turn_stride", C.c_int64), ("state_env_stride", C.c_int64),
        ("scalar_turn_stride", C.c_int64), ("scalar_env_stride", C.c_int64),
        ("seed", C.c_uint64), ("draw", C.c_uint64),
        ("n_frames", C.c_int32), ("src_type", C.c_int32), ("act_type", C.c_int32), ("reserved", C.c_int32),
    ]


class SgwReturnsDesc(C.Structure):
    """Mirror of ``struct sgw_returns_desc`` (include/sgw.h): one ``sgw_returns`` call."""

    _fields_ = [
        ("rewards", C.c_void_p), ("dones", C.c_void_p), ("out_returns", C.c_void_p), ("out_normalized", C.c_void_p),
        ("out_stats", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("first", C.c_int64), ("count", C.c_int64), ("capacity", C.c_int64), ("cols", C.c_int64),
        ("turn_stride", C.c_int64), ("col_stride", C.c_int64),
        ("gamma", C.c_double),
        ("normalize", C.c_int32), ("out_type", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwPolicyDesc(C.Structure):
    """Mirror of ``struct sgw_policy_desc`` (include/sgw.h): one ``sgw_policy_sample`` call."""

    _fields_ = [
        ("dist", C.c_void_p), ("idx", C.c_void_p), ("out_actions", C.c_void_p), ("out_log_probs", C.c_void_p), ("out_entropy", C.c_void_p),
        ("n", C.c_int64), ("num_envs", C.c_int64), ("row_stride", C.c_int64),
        ("seed", C.c_uint64), ("first_env", C.c_uint64),
        ("epoch", C.c_uint32), ("turn", C.c_uint32),
        ("num_actions", C.c_int32), ("agent0", C.c_int32), ("dist_type", C.c_int32), ("mode", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwPpoLossDesc(C.Structure):
    """Mirror of ``struct sgw_ppo_loss_desc`` (include/sgw.h): one ``sgw_ppo_loss`` call."""

    _fields_ = [
        ("dist", C.c_void_p), ("values", C.c_void_p), ("actions", C.c_void_p), ("old_log_probs", C.c_void_p), ("returns", C.c_void_p),
        ("out_grad_dist", C.c_void_p), ("out_grad_values", C.c_void_p), ("out_row_terms", C.c_void_p), ("out_terms", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("n", C.c_int64), ("row_stride", C.c_int64),
        ("eps_clip", C.c_double), ("entropy_coef", C.c_double), ("value_coef", C.c_double),
        ("num_actions", C.c_int32), ("dist_type", C.c_int32), ("mode", C.c_int32), ("value_type", C.c_int32), ("action_type", C.c_int32),
        ("returns_type", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwIqnLossDesc(C.Structure):
    """Mirror of ``struct sgw_iqn_loss_desc`` (include/sgw.h): one ``sgw_iqn_loss`` call."""

    _fields_ = [
        ("q_next_local", C.c_void_p), ("q_next_target", C.c_void_p), ("q_expected", C.c_void_p), ("taus", C.c_void_p),
        ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p), ("valid", C.c_void_p),
        ("out_terms", C.c_void_p), ("out_grad_expected", C.c_void_p), ("out_next_actions", C.c_void_p), ("out_row_terms", C.c_void_p),
        ("out_td_error", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("n", C.c_int64),
        ("discount", C.c_double),
        ("num_quantiles", C.c_int32), ("num_actions", C.c_int32), ("action_type", C.c_int32), ("valid_type", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwIqnForwardDesc(C.Structure):
    """Mirror of ``struct sgw_iqn_forward_desc`` (include/sgw.h): one ``sgw_iqn_forward`` call."""

    _fields_ = [
        ("states", C.c_void_p),
        ("w_head", C.c_void_p), ("b_head", C.c_void_p), ("w_cos", C.c_void_p), ("b_cos", C.c_void_p), ("w_ff", C.c_void_p), ("b_ff", C.c_void_p),
        ("w_adv", C.c_void_p), ("b_adv", C.c_void_p), ("w_val", C.c_void_p), ("b_val", C.c_void_p),
        ("taus", C.c_void_p), ("idx", C.c_void_p),
        ("out_qvalues", C.c_void_p), ("out_quantiles", C.c_void_p), ("out_taus", C.c_void_p), ("out_cos", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("n", C.c_int64), ("state_stride", C.c_int64), ("num_envs", C.c_int64),
        ("seed", C.c_uint64), ("first_env", C.c_uint64),
        ("epoch", C.c_uint32), ("turn", C.c_uint32),
        ("in_features", C.c_int32), ("layer_size", C.c_int32), ("num_quantiles", C.c_int32), ("num_actions", C.c_int32), ("n_cos", C.c_int32),
        ("state_type", C.c_int32), ("agent0", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwIqnBackwardDesc(C.Structure):
    """Mirror of ``struct sgw_iqn_backward_desc`` (include/sgw.h): one ``sgw_iqn_backward`` call."""

    _fields_ = [
        ("states", C.c_void_p),
        ("w_head", C.c_void_p), ("b_head", C.c_void_p), ("w_cos", C.c_void_p), ("b_cos", C.c_void_p), ("w_ff", C.c_void_p), ("b_ff", C.c_void_p),
        ("w_adv", C.c_void_p), ("b_adv", C.c_void_p), ("w_val", C.c_void_p), ("b_val", C.c_void_p),
        ("taus", C.c_void_p), ("h", C.c_void_p), ("grad_quantiles", C.c_void_p),
        ("out_w_head", C.c_void_p), ("out_b_head", C.c_void_p), ("out_w_cos", C.c_void_p), ("out_b_cos", C.c_void_p), ("out_w_ff", C.c_void_p),
        ("out_b_ff", C.c_void_p), ("out_w_adv", C.c_void_p), ("out_b_adv", C.c_void_p), ("out_w_val", C.c_void_p), ("out_b_val", C.c_void_p),
        ("out_grad_h", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("n", C.c_int64), ("state_stride", C.c_int64),
        ("in_features", C.c_int32), ("layer_size", C.c_int32), ("num_quantiles", C.c_int32), ("num_actions", C.c_int32), ("n_cos", C.c_int32),
        ("state_type", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwAdamTensor(C.Structure):
    """Mirror of ``struct sgw_adam_tensor`` (include/sgw.h): one tensor of an ``sgw_adam_plan`` call."""

    _fields_ = [
        ("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("target", C.c_void_p),
        ("numel", C.c_int64),
        ("lr", C.c_double),
        ("reserved", C.c_int64),
    ]


class SgwAdamPlanInfo(C.Structure):
    """Mirror of ``struct sgw_adam_plan_info``."""

    _fields_ = [("num_chunks", C.c_int64), ("workspace_bytes", C.c_int64), ("image_bytes", C.c_int64), ("total_numel", C.c_int64)]


class SgwAdamStepState(C.Structure):
    """Mirror of ``struct sgw_adam_step_state``: the device's step count and the running products of the betas."""

    _fields_ = [("step", C.c_int64), ("beta1_pow", C.c_double), ("beta2_pow", C.c_double)]


class SgwAdamStepDesc(C.Structure):
    """Mirror of ``struct sgw_adam_step_desc``: one ``sgw_adam_step`` call."""

    _fields_ = [
        ("plan", C.c_void_p),
        ("plan_bytes", C.c_int64),
        ("clip_coef", C.c_void_p), ("step_state", C.c_void_p), ("out_norm", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("num_tensors", C.c_int64), ("num_chunks", C.c_int64),
        ("step", C.c_int64),
        ("max_norm", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("tau", C.c_double),
        ("dtype", C.c_int32), ("clip_mode", C.c_int32), ("flags", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwNoisyJob(C.Structure):
    """Mirror of ``struct sgw_noisy_job``: one tensor of an ``sgw_noisy_weights`` call."""

    _fields_ = [
        ("weight", C.c_void_p), ("sigma", C.c_void_p), ("eps_in", C.c_void_p), ("grad_eff", C.c_void_p),
        ("out_eff", C.c_void_p), ("out_eps", C.c_void_p), ("out_grad_sigma", C.c_void_p),
        ("count", C.c_int64),
        ("tensor_id", C.c_int32), ("reserved", C.c_int32),
    ]


class SgwNoisyWeightsDesc(C.Structure):
    """Mirror of ``struct sgw_noisy_weights_desc``: one ``sgw_noisy_weights`` call."""

    _fields_ = [
        ("jobs", SgwNoisyJob * NOISY_MAX_JOBS),
        ("seed", C.c_uint64), ("draw", C.c_uint64),
        ("num_jobs", C.c_int32), ("mode", C.c_int32),
        ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]


class SgwLearnClock(C.Structure):
    """Mirror of ``struct sgw_learn_clock``: what the ``*_clocked`` calls read in DEVICE memory (the host builds its image and uploads it)."""

    _fields_ = [("count", C.c_uint64), ("num_starts", C.c_int64), ("reserved", C.c_uint64 * 2)]


_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SGW_LIB") or os.path.join(_HERE, "csrc", "libsgw.so")   # SGW_LIB: diagnostic builds (tools/)

_rc, _vp, _i32, _u32, _i64, _f64 = C.c_int, C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_double    # (every data pointer is a void *)
_vpp, _cfgp = C.POINTER(C.c_void_p), C.POINTER(SgwConfig)

# every symbol include/sgw.h declares: name -> (restype, argtypes); tests/test_abi.py compares each with the header's declaration
PROTOTYPES = {
    "sgw_create": (_rc, [_cfgp, C.POINTER(_vp)]),
    "sgw_destroy": (None, [_vp]),
    "sgw_reset": (_rc, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "sgw_observe": (_rc, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "sgw_step": (_rc, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _i32, _i32, _u32, _vp]),
    "sgw_rollout": (_rc, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _i64, _i64, _i64, _u32, _vp]),
    "sgw_reduce_metrics": (_rc, [_vp, _vp, _vp, _vp]),
    "sgw_random_actions": (_rc, [_vp, _vp, _u32, _u32, _vp]),
    "sgw_set_obs_format": (_rc, [_vp, C.c_int]),
    "sgw_bind_agent_state": (_rc, [_vp, _vp, _vp]),
    "sgw_bind_agent_dir": (_rc, [_vp, _vp]),
    "sgw_bind_target_types": (_rc, [_vp, _vp]),
    "sgw_bind_encounters": (_rc, [_vp, _vp, _vp, _i32]),
    "sgw_init_agent_state": (_rc, [_vp, _vp, _vp]),
    "sgw_get_status": (_rc, [_vp, C.POINTER(_i32), _vp]),
    "sgw_obs_elems_per_env": (_i64, [_cfgp]),
    "sgw_grid_bytes_per_env": (_i64, [_cfgp]),
    "sgw_algorithmic_bytes_per_env_step": (_i64, [_cfgp]),
    "sgw_set_timing": (_rc, [_vp, C.c_int]),
    "sgw_get_step_time_ms": (_rc, [_vp, C.POINTER(_f64), C.POINTER(_i64)]),
    "sgw_get_step_times_ms": (_rc, [_vp, C.POINTER(C.c_float), _i64, C.POINTER(_i64)]),
    "sgw_set_auto_reset": (_rc, [_vp, _u32, _vp]),
    "sgw_set_wg_per_cu": (_rc, [_vp, C.c_int]),
    "sgw_launch_info": (_rc, [_vp, C.c_char_p, _i64]),
    "sgw_observe_full": (_rc, [_vp, _vp, _vp, _vp]),
    "sgw_capabilities": (_rc, [_vp]),
    "sgw_observe_rows": (_rc, [_vp, _vp, _vp, _vpp, _i64, _i32, _i32, _vp]),
    "sgw_sweep_observe_rows": (_rc, [_vp, _vp, _vp, _vpp, _i64, _u32, _u32, _u32, _vp]),
    "sgw_act": (_rc, [_vp, _vp, _vp, _vp, _vpp, _i64, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "sgw_set_option": (_rc, [_vp, C.c_char_p, C.c_char_p]),
    "sgw_plan": (_rc, [_cfgp, _i32, _i64, C.POINTER(SgwPlan)]),
    "sgw_jit_compile": (_rc, [C.c_char_p, C.c_char_p, C.c_char_p, _i64]),
    "sgw_jit_stats": (_rc, [C.POINTER(_f64)]),
    "sgw_bind_row_tail": (_rc, [_vp, C.c_int, C.c_int, _vp]),
    "sgw_turn_bind": (_rc, [_vp, C.POINTER(SgwTurnRows)]),
    "sgw_turn_set": (_rc, [_vp, _u32, _u32, _vp]),
    "sgw_turn_begin": (_rc, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "sgw_turn_act": (_rc, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp]),
    "sgw_turn_begin_rows": (_rc, [_vp, _vp, _vp, _vp, _vp, _vp, _vpp, _i64, _u32, _vp]),
    "sgw_turn_act_rows": (_rc, [_vp, _vp, _vp, _vp, _vpp, _i64, _vp, _vp, _i32, _vp, _i32, _vp]),
    "sgw_turn_end": (_rc, [_vp, _vp, _vp]),
    "sgw_turn_state": (_rc, [_vp, C.POINTER(_u32), C.POINTER(_i64), _vp]),
    "sgw_turn_resolve": (_rc, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp]),
    "sgw_gather_rows": (_rc, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "sgw_verify_rows": (_rc, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "sgw_apply_actions": (_rc, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "sgw_choose_actions": (_rc, [_vp, _vp, _vp, _i64, _u32, _u32, _vp, _vp]),
    "sgw_turn_prev_rows": (_rc, [_vp, _i32, _i32, _vp, _vp]),
    "sgw_turn_epsilon": (_rc, [_vp, _i32, _f64, _vp]),
    "sgw_render": (_rc, [C.POINTER(SgwRenderDesc), _vp]),
    "sgw_sample": (_rc, [C.POINTER(SgwSampleDesc), _vp]),
    "sgw_returns": (_rc, [C.POINTER(SgwReturnsDesc), _vp]),
    "sgw_returns_workspace_bytes": (_i64, [_i64, _i64]),
    "sgw_policy_sample": (_rc, [C.POINTER(SgwPolicyDesc), _vp]),
    "sgw_turn_policy_sample": (_rc, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "sgw_ppo_loss": (_rc, [C.POINTER(SgwPpoLossDesc), _vp]),
    "sgw_ppo_loss_workspace_bytes": (_i64, [_i64]),
    "sgw_iqn_loss": (_rc, [C.POINTER(SgwIqnLossDesc), _vp]),
    "sgw_iqn_loss_workspace_bytes": (_i64, [_i64, _i32]),
    "sgw_iqn_forward": (_rc, [C.POINTER(SgwIqnForwardDesc), _vp]),
    "sgw_iqn_forward_workspace_bytes": (_i64, [_i64, _i32]),
    "sgw_turn_iqn_forward": (_rc, [_vp, _i32, C.POINTER(SgwIqnForwardDesc), _vp]),
    "sgw_iqn_backward": (_rc, [C.POINTER(SgwIqnBackwardDesc), _vp]),
    "sgw_iqn_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "sgw_noisy_weights": (_rc, [C.POINTER(SgwNoisyWeightsDesc), _vp]),
    "sgw_noisy_weights_clocked": (_rc, [C.POINTER(SgwNoisyWeightsDesc), _vp, _vp]),
    "sgw_iqn_forward_clocked": (_rc, [C.POINTER(SgwIqnForwardDesc), _vp, _vp]),
    "sgw_sample_clocked": (_rc, [C.POINTER(SgwSampleDesc), _vp, _vp]),
    "sgw_learn_clock_advance": (_rc, [_vp, _vp]),
    "sgw_adam_plan_bytes": (_i64, [_i64, _i64]),
    "sgw_adam_plan": (_rc, [C.POINTER(SgwAdamTensor), _i64, _i32, _vp, _i64, C.POINTER(SgwAdamPlanInfo)]),
    "sgw_adam_step": (_rc, [C.POINTER(SgwAdamStepDesc), _vp]),
    "sgw_last_error": (C.c_char_p, []),
    "sgw_version": (C.c_char_p, []),
}
EXPORTS = tuple(PROTOTYPES)

_lib = None
_torch = None        # torch, kept by load() (imported there, not here: importing this module stays free of it)
raw_stream = None    # load(): raw_stream(index) = the caller's current stream on device `index`, as the integer the library takes


class SgwError(RuntimeError):
    pass


def _hip_runtimes_mapped():
    paths = set()
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64" in line:
                    paths.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    return sorted(paths)


def load():
    """Load libsgw.so (after torch, so that it binds to torch's HIP runtime)."""
    global _lib, _torch
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise SgwError(
            f"HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the step/observe path."
        )
    import torch  # (maps torch's libamdhip64 first; libsgw.so then resolves to the same soname)

    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    rts = _hip_runtimes_mapped()
    if len(rts) > 1:
        raise SgwError(f"two HIP runtimes are mapped in this process ({rts}); stream handles would not be shared")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib, _torch = lib, torch
    global raw_stream
    # the private accessor PyTorch's own compilers use where it exists: the public one costs ~5 us per call, a third of a small-batch step
    raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda index: torch.cuda.current_stream(index).cuda_stream)
    # tools pass dispatcher options to child processes as SGW_OPTIONS="key=value,key=value": read HERE, by the Python
    # tooling -- the library itself reads no environment variable except SGW_DEBUG
    for item in filter(None, os.environ.get("SGW_OPTIONS", "").replace(";", ",").split(",")):
        key, _, value = item.partition("=")
        set_option(key.strip(), value.strip())
        _opt_baseline[key.strip()] = value.strip()
    return lib


_opt_values = {}      # process-wide options as they stand (key -> text), mirrored here so that a block can put back what it found
_opt_baseline = {}    # ... as SGW_OPTIONS set them when the library was loaded


def set_option(key, value=None, engine=None) -> None:
    """``sgw_set_option``: a dispatcher knob (``sorrel_amd/csrc/options.h``) for engines created from now on, or -- the live
    keys only -- for one engine handle.  ``value=None`` restores the key's default, ``key=None`` all of them."""
    lib = load()
    k = None if key is None else str(key).encode()
    v = None if value is None else str(int(value) if isinstance(value, bool) else value).encode()
    check(lib.sgw_set_option(engine, k, v))
    if engine is None:
        if key is None:
            _opt_values.clear()
        elif value is None:
            _opt_values.pop(str(key), None)
        else:
            _opt_values[str(key)] = v.decode()


def get_option(key):
    """The process-wide value last set for ``key`` through this module (text), or None while it stands at the library's default."""
    return _opt_values.get(str(key))


def reset_options() -> None:
    """Every process-wide option back to where the process started: the library's defaults plus what ``SGW_OPTIONS`` asked for."""
    set_option(None)
    for k, v in _opt_baseline.items():
        set_option(k, v)


class options:
    """``with options(group=16, jit=0): ...`` -- process-wide options for the engines created inside the block; on exit every key goes
    back to the value it had on entry (not to the library default: blocks nest, and what ``SGW_OPTIONS`` set survives them)."""

    def __init__(self, **kw):
        self.kw = kw
        self.before = {}

    def __enter__(self):
        self.before = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            set_option(k, v)
        return False


def plan(cfg: "SgwConfig", num_cus: int = 256, lds_per_workgroup: int = 160 * 1024) -> dict:
    """``sgw_plan``: kernel family, LDS layout, staging and instances ``sgw_create`` would choose -- no device needed."""
    out = SgwPlan()
    check(load().sgw_plan(C.byref(cfg), num_cus, lds_per_workgroup, C.byref(out)))
    return out.as_dict()


def jit_compile(instance: str, arch: str = "gfx950") -> str:
    """``sgw_jit_compile``: the cache file of one specialised instance, compiled now if the cache does not hold it (no device needed)."""
    buf = C.create_string_buffer(1024)
    check(load().sgw_jit_compile(instance.encode(), arch.encode(), buf, 1024))
    return buf.value.decode()


def jit_code_object(path: str):
    """(lowered kernel name, code object bytes) of a cache file."""
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[:8] == b"SGWJIT2\n", path
    n = int.from_bytes(data[8:12], "little")
    return data[12:12 + n].decode(), data[12 + n + 16:]          # (u64 size + u64 checksum in front of the code object)


def jit_stats() -> dict:
    buf = (C.c_double * 6)()
    check(load().sgw_jit_stats(buf))
    return dict(compiled=int(buf[0]), disk_hits=int(buf[1]), mem_hits=int(buf[2]), failed=int(buf[3]),
                compile_ms=float(buf[4]), load_ms=float(buf[5]))


_functions = {}     # launch(): the library's functions by name, looked up once (the small shapes are bound by the host)


class _NoSwitch:
    """Context manager that does nothing: the device is already the current one."""

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def on_device(index: int):
    """Context that makes device ``index`` current; a no-op object when it already is (the usual case -- entering
    ``torch.cuda.device`` costs several microseconds)."""
    return _NO_SWITCH if _torch.cuda.current_device() == index else _torch.cuda.device(index)


def call(index: int, fn, *args) -> None:
    """THE library call: ``fn(*args)`` with device ``index`` current for it (the library launches on the current device; the pointers
    and the stream among ``args`` belong to that device), a non-zero return code raised as ``check`` raises it.  No context manager
    where the device is current already, nothing allocated, no synchronisation: legal inside a stream capture."""
    if _torch.cuda.current_device() == index:
        code = fn(*args)
    else:
        with _torch.cuda.device(index):
            code = fn(*args)
    if code:
        check(code)


def launch(name: str, desc, device, *leading, clock=None) -> None:
    """One descriptor call ``name(*leading, &desc, stream)`` on ``device``'s current stream, through ``call``.  ``clock``: the device address
    of an ``sgw_learn_clock``; the call is then the clocked twin ``name_clocked(*leading, &desc, clock, stream)``."""
    if clock is not None:
        name += "_clocked"
    fn = _functions.get(name)
    if fn is None:
        fn = _functions[name] = getattr(load(), name)
    index = device.index
    if index is None:
        index = _torch.cuda.current_device()
    if clock is None:
        call(index, fn, *leading, C.byref(desc), raw_stream(index))
    else:
        call(index, fn, *leading, C.byref(desc), clock, raw_stream(index))


def workspace(nbytes: int, device):
    """The float64 tensor a descriptor's ``workspace`` / ``workspace_bytes`` point at: ``nbytes`` (what a ``sgw_*_workspace_bytes`` gave:
    a negative value is its error code) rounded up, at least one element."""
    import torch

    if nbytes < 0:
        check(int(nbytes))
    return torch.empty((max((int(nbytes) + 7) // 8, 1),), dtype=torch.float64, device=device)


def float_code(dtype) -> int:
    """``POLICY_F32`` / ``POLICY_F64`` of a float tensor's torch dtype (every descriptor's ``*_type`` of a float tensor), by its width."""
    return POLICY_F64 if dtype.itemsize == 8 else POLICY_F32


def action_code(dtype) -> int:
    """``PPO_ACT_I64`` / ``PPO_ACT_U8`` of an action tensor's torch dtype (the losses' ``action_type``), by its width."""
    return PPO_ACT_U8 if dtype.itemsize == 1 else PPO_ACT_I64


def check(rc: int) -> None:
    if rc != OK:
        msg = load().sgw_last_error().decode("utf-8", "replace")
        if rc == EINVAL:
            raise ValueError(msg)   # the reference raises ValueError/TypeError for bad specs
        raise SgwError(f"sgw error {rc}: {msg}")
