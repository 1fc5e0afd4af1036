"""ctypes binding of the C ABI in include/resco_sim.h (resco_amd/csrc/libresco_sim.so).

This is the only gateway to the simulator: there is NO CPU fallback.  If the HIP library is
missing or no MI355X is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

from ._abi import DemandStruct, Fma2cRewardTableStruct, Fma2cTrainStruct, ParamsStruct, PPOTrainStruct, RolloutStruct, TrainStruct, pack_scenario

_HERE = os.path.dirname(os.path.abspath(__file__))
# RESCO_SIM_LIB: another build of the same HIP library (A/B variants compiled with different -D switches, tools/ab.py)
LIB_PATH = os.environ.get('RESCO_SIM_LIB') or os.path.join(_HERE, 'csrc', 'libresco_sim.so')

BUFFERS = ['lane_agg', 'drq_norm', 'phase', 'mplight', 'wave', 'wait', 'wait_norm', 'pressure', 'queue_sum',
           'queue_max', 'actions', 'env', 'tls', 'veh_pos', 'veh_speed', 'veh_accel', 'veh_tloss', 'veh_lane',
           'veh_trip', 'veh_cursor', 'veh_swait', 'veh_rwait', 'veh_depart', 'veh_owner', 'stats', 'drq_norm_f16',
           'veh_sf', 'veh_wtot', 'trip_log', 'dep_next', 'veh_coop', 'veh_cooplead', 'arrivals', 'departures',
           'mplight_full', 'lane_arrivals', 'veh_coop_odd', 'veh_cooplead_odd', 'veh_mail']
BUF_ID = {n: i for i, n in enumerate(BUFFERS)}
OUTPUT_GROUPS = ('lane_agg', 'drq_norm', 'drq_norm_f16', 'lane_arrivals', 'mplight', 'wave', 'mplight_full', 'veh_accel')
_NP_DTYPES = [np.float32, np.int32, np.uint16, np.uint8, np.float16, np.int64, np.uint32]
_TYPESTR = ['<f4', '<i4', '<u2', '|u1', '<f2', '<i8', '<u4']
STAT_KEYS = ['inserted', 'arrived', 'sum_duration', 'sum_depart_delay', 'sum_waiting', 'sum_time_loss_q10',
             'active', 'pending', 'active_ticks', 'ticks', 'cap_blocked', 'invariant']
TRIP_NONE = 0xFFFF

# every symbol include/resco_sim.h declares
ABI_SYMBOLS = ['rs_create', 'rs_destroy', 'rs_last_error', 'rs_reset', 'rs_step', 'rs_sync', 'rs_reinit_signals', 'rs_ticks', 'rs_step_sim', 'rs_set_outputs', 'rs_act_random',
               'rs_act_maxwave', 'rs_get_buffer', 'rs_read_buffer', 'rs_stats', 'rs_snapshot', 'rs_restore',
               'rs_snapshot_free', 'rs_timing', 'rs_timing_read', 'rs_set_seed', 'rs_phase_profile', 'rs_info',
               'rs_idqn_create', 'rs_idqn_act', 'rs_idqn_set_device_weights', 'rs_idqn_set_lanes', 'rs_idqn_destroy', 'rs_group_step',
               'rs_default_block', 'rs_mplight_create', 'rs_mplight_act', 'rs_mplight_set_device_weights', 'rs_mplight_destroy',
               'rs_ippo_act', 'rs_group_rollout', 'rs_ppo_gae',
               'rs_ppo_create', 'rs_ppo_grad', 'rs_ppo_step', 'rs_ppo_fit', 'rs_ppo_steps', 'rs_ppo_set_steps', 'rs_ppo_destroy',
               'rs_dqn_create', 'rs_dqn_sample', 'rs_dqn_grad', 'rs_dqn_step', 'rs_dqn_update', 'rs_dqn_steps', 'rs_dqn_set_steps',
               'rs_dqn_set_target', 'rs_dqn_get_target', 'rs_dqn_destroy',
               'rs_dqn_set_priorities', 'rs_dqn_get_priorities', 'rs_dqn_per_rebuild', 'rs_dqn_per_fill', 'rs_dqn_per_commit',
               'rs_mplight_dqn_create', 'rs_mplight_dqn_sample', 'rs_mplight_dqn_grad', 'rs_mplight_dqn_step', 'rs_mplight_dqn_update',
               'rs_mplight_dqn_steps', 'rs_mplight_dqn_set_steps', 'rs_mplight_dqn_set_target', 'rs_mplight_dqn_get_target', 'rs_mplight_dqn_destroy',
               'rs_mplight_dqn_set_priorities', 'rs_mplight_dqn_get_priorities', 'rs_mplight_dqn_per_rebuild', 'rs_mplight_dqn_per_fill',
               'rs_mplight_dqn_per_commit',
               'rs_mplight_multi_create', 'rs_mplight_multi_sample', 'rs_mplight_multi_grad', 'rs_mplight_multi_step', 'rs_mplight_multi_update',
               'rs_mplight_multi_sync_target', 'rs_mplight_multi_steps', 'rs_mplight_multi_set_steps', 'rs_mplight_maps_set_target',
               'rs_mplight_maps_get_target', 'rs_mplight_multi_destroy',
               'rs_idqn_pack_weights', 'rs_dqn_sync_target', 'rs_mplight_dqn_sync_target', 'rs_group_train',
               'rs_ppo_perm', 'rs_ippo_pack_weights', 'rs_group_ppo_train', 'rs_info_kernel', 'rs_set_demand', 'rs_demand_info']

# the FMA2C entry points (include/resco_sim.h: rs_fma2c_*)
FMA2C_SYMBOLS = ['rs_fma2c_create', 'rs_fma2c_act', 'rs_fma2c_value', 'rs_fma2c_reset', 'rs_fma2c_set_device_weights', 'rs_fma2c_buffer',
                 'rs_fma2c_destroy', 'rs_fma2c_learn_create', 'rs_fma2c_learn_grad', 'rs_fma2c_learn_step', 'rs_fma2c_learn_update',
                 'rs_fma2c_learn_reset', 'rs_fma2c_learn_buffer', 'rs_fma2c_learn_destroy', 'rs_fma2c_record']
# the FMA2C training loop (include/resco_sim.h: rs_group_fma2c_train)
FMA2C_LOOP_SYMBOLS = ['rs_group_fma2c_train']

_lib = None


def bind(L):
    """ctypes signatures of the C ABI (include/resco_sim.h) on an opened library."""
    vp, i32, u32, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    L.rs_create.argtypes = [vp, vp, i32, i32, i32, i32, C.POINTER(vp)]
    L.rs_destroy.argtypes = [vp]
    L.rs_destroy.restype = None
    L.rs_last_error.argtypes = [vp]
    L.rs_last_error.restype = C.c_char_p
    L.rs_reset.argtypes = [vp, vp]
    L.rs_step.argtypes = [vp, vp, i32, vp]
    L.rs_sync.argtypes = [vp]
    L.rs_ticks.argtypes = [vp, i32, vp]
    L.rs_step_sim.argtypes = [vp, i32, vp]
    L.rs_set_outputs.argtypes = [vp, C.c_uint64]
    L.rs_reinit_signals.argtypes = [vp, vp]
    L.rs_act_random.argtypes = [vp, C.c_uint32, vp]
    L.rs_act_maxwave.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.rs_get_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(i32), C.POINTER(i32)]
    L.rs_read_buffer.argtypes = [vp, i32, vp, C.c_int64]
    L.rs_stats.argtypes = [vp, vp]
    L.rs_snapshot.argtypes = [vp, C.POINTER(vp)]
    L.rs_restore.argtypes = [vp, vp]
    L.rs_snapshot_free.argtypes = [vp, vp]
    L.rs_snapshot_free.restype = None
    L.rs_timing.argtypes = [vp, i32]
    L.rs_timing_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i32)]
    L.rs_set_seed.argtypes = [vp, C.c_uint32]
    L.rs_phase_profile.argtypes = [vp, i32, vp]
    L.rs_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.rs_group_step.argtypes = [vp, i32, vp, i32]
    if hasattr(L, 'rs_info_kernel'):
        L.rs_info_kernel.argtypes = [vp]
        L.rs_info_kernel.restype = C.c_char_p
    if hasattr(L, 'rs_set_demand'):         # (tests/hostemu exports no per-environment demand)
        L.rs_set_demand.argtypes = [vp, i32, vp, vp]
        L.rs_demand_info.argtypes = [vp, C.POINTER(i32), vp]
    if hasattr(L, 'rs_idqn_create'):
        L.rs_idqn_create.argtypes = [i32, i32, i32] + [vp] * 9 + [C.POINTER(vp)]
        L.rs_idqn_act.argtypes = [vp, vp, i32, i32, i32, f32, u32, u32, vp, vp, vp, vp]
        L.rs_idqn_set_lanes.argtypes = [vp, vp]
        L.rs_idqn_set_device_weights.argtypes = [vp] * 9
        L.rs_idqn_destroy.argtypes = [vp]
        L.rs_idqn_destroy.restype = None
    if hasattr(L, 'rs_mplight_create'):
        L.rs_mplight_create.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, C.POINTER(vp)]
        L.rs_mplight_act.argtypes = [vp, vp, i32, i32, f32, u32, u32, vp, vp, vp, vp, vp]
        L.rs_mplight_set_device_weights.argtypes = [vp, vp]
        L.rs_mplight_destroy.argtypes = [vp]
        L.rs_mplight_destroy.restype = None
    if hasattr(L, 'rs_group_rollout'):
        L.rs_ippo_act.argtypes = [vp, vp, i32, i32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.rs_group_rollout.argtypes = [vp, i32, vp, vp, i32, i32]
        L.rs_ppo_gae.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp]
    if hasattr(L, 'rs_ppo_create'):
        L.rs_ppo_create.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        L.rs_ppo_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
        L.rs_ppo_step.argtypes = [vp, vp]
        L.rs_ppo_fit.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, vp, vp]
        L.rs_ppo_steps.argtypes = [vp]
        L.rs_ppo_steps.restype = C.c_int64
        if hasattr(L, 'rs_ppo_set_steps'):      # (a host emulation may not have it)
            L.rs_ppo_set_steps.argtypes = [vp, C.c_int64]
        L.rs_ppo_destroy.argtypes = [vp]
        L.rs_ppo_destroy.restype = None
    if hasattr(L, 'rs_dqn_create'):
        L.rs_dqn_create.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        L.rs_dqn_sample.argtypes = [vp, vp, i32, u32, u32, vp, vp]
        L.rs_dqn_grad.argtypes = [vp, vp, vp, i32, vp, vp]
        L.rs_dqn_step.argtypes = [vp, vp]
        L.rs_dqn_update.argtypes = [vp, vp, i32, u32, i32, vp, vp]
        L.rs_dqn_steps.argtypes = [vp]
        L.rs_dqn_steps.restype = C.c_int64
        if hasattr(L, 'rs_dqn_set_steps'):      # (a host emulation may not have it)
            L.rs_dqn_set_steps.argtypes = [vp, C.c_int64]
        if hasattr(L, 'rs_dqn_set_target'):     # (a host emulation may not have them)
            L.rs_dqn_set_target.argtypes = [vp, i32, i32]
            L.rs_dqn_get_target.argtypes = [vp, vp, vp]
        if hasattr(L, 'rs_dqn_set_priorities'):     # (a host emulation may not have them)
            L.rs_dqn_set_priorities.argtypes = [vp, vp]
            L.rs_dqn_get_priorities.argtypes = [vp, vp, vp]
            L.rs_dqn_per_rebuild.argtypes = [vp, vp]
            L.rs_dqn_per_fill.argtypes = [vp, i32, vp]
            L.rs_dqn_per_commit.argtypes = [vp, vp, vp, i32, vp]
        L.rs_dqn_destroy.argtypes = [vp]
        L.rs_dqn_destroy.restype = None
    if hasattr(L, 'rs_mplight_dqn_create'):
        L.rs_mplight_dqn_create.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        L.rs_mplight_dqn_sample.argtypes = [vp, vp, i32, u32, u32, vp, vp]
        L.rs_mplight_dqn_grad.argtypes = [vp, vp, vp, i32, vp, vp]
        L.rs_mplight_dqn_step.argtypes = [vp, vp]
        L.rs_mplight_dqn_update.argtypes = [vp, vp, i32, u32, i32, vp, vp]
        L.rs_mplight_dqn_steps.argtypes = [vp]
        L.rs_mplight_dqn_steps.restype = C.c_int64
        if hasattr(L, 'rs_mplight_dqn_set_steps'):      # (a host emulation may not have it)
            L.rs_mplight_dqn_set_steps.argtypes = [vp, C.c_int64]
        if hasattr(L, 'rs_mplight_dqn_set_target'):     # (a host emulation may not have them)
            L.rs_mplight_dqn_set_target.argtypes = [vp, i32, i32]
            L.rs_mplight_dqn_get_target.argtypes = [vp, vp, vp]
        if hasattr(L, 'rs_mplight_dqn_set_priorities'):     # (a host emulation may not have them)
            L.rs_mplight_dqn_set_priorities.argtypes = [vp, vp]
            L.rs_mplight_dqn_get_priorities.argtypes = [vp, vp, vp]
            L.rs_mplight_dqn_per_rebuild.argtypes = [vp, vp]
            L.rs_mplight_dqn_per_fill.argtypes = [vp, i32, vp]
            L.rs_mplight_dqn_per_commit.argtypes = [vp, vp, vp, i32, vp]
        L.rs_mplight_dqn_destroy.argtypes = [vp]
        L.rs_mplight_dqn_destroy.restype = None
    if hasattr(L, 'rs_mplight_multi_create'):
        L.rs_mplight_multi_create.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        L.rs_mplight_multi_sample.argtypes = [vp, vp, i32, u32, u32, vp, vp, vp]
        L.rs_mplight_multi_grad.argtypes = [vp, vp, vp, vp, i32, vp, vp]
        L.rs_mplight_multi_step.argtypes = [vp, vp]
        L.rs_mplight_multi_update.argtypes = [vp, vp, i32, u32, i32, vp, vp]
        L.rs_mplight_multi_sync_target.argtypes = [vp, vp]
        L.rs_mplight_multi_steps.argtypes = [vp]
        L.rs_mplight_multi_steps.restype = C.c_int64
        L.rs_mplight_multi_set_steps.argtypes = [vp, C.c_int64]
        if hasattr(L, 'rs_mplight_maps_set_target'):   # (a host emulation may not have them)
            L.rs_mplight_maps_set_target.argtypes = [vp, i32, i32]
            L.rs_mplight_maps_get_target.argtypes = [vp, vp, vp]
        L.rs_mplight_multi_destroy.argtypes = [vp]
        L.rs_mplight_multi_destroy.restype = None
    if hasattr(L, 'rs_group_train'):
        L.rs_idqn_pack_weights.argtypes = [vp, vp, vp]
        L.rs_dqn_sync_target.argtypes = [vp, vp]
        L.rs_mplight_dqn_sync_target.argtypes = [vp, vp]
        L.rs_group_train.argtypes = [vp, i32, vp, i32]
    if hasattr(L, 'rs_group_ppo_train'):
        L.rs_ppo_perm.argtypes = [i32, i32, u32, u32, vp, vp]
        L.rs_ippo_pack_weights.argtypes = [vp, vp, vp]
        L.rs_group_ppo_train.argtypes = [vp, i32, vp, i32]
    if hasattr(L, 'rs_fma2c_create'):
        L.rs_fma2c_create.argtypes = [i32, vp, vp, i32, C.POINTER(vp)]
        L.rs_fma2c_act.argtypes = [vp, vp, i32, i32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.rs_fma2c_value.argtypes = [vp, vp, i32, i32, vp, vp]
        L.rs_fma2c_reset.argtypes = [vp, i32, i32, i32, vp]
        L.rs_fma2c_set_device_weights.argtypes = [vp, vp]
        L.rs_fma2c_buffer.argtypes = [vp, i32, C.POINTER(vp)]
        L.rs_fma2c_destroy.argtypes = [vp]
        L.rs_fma2c_destroy.restype = None
    if hasattr(L, 'rs_fma2c_learn_create'):
        L.rs_fma2c_learn_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
        L.rs_fma2c_learn_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
        L.rs_fma2c_learn_step.argtypes = [vp, vp]
        L.rs_fma2c_learn_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
        L.rs_fma2c_learn_reset.argtypes = [vp, vp]
        L.rs_fma2c_learn_buffer.argtypes = [vp, i32, C.POINTER(vp)]
        L.rs_fma2c_learn_destroy.argtypes = [vp]
        L.rs_fma2c_learn_destroy.restype = None
    if hasattr(L, 'rs_group_fma2c_train'):
        L.rs_fma2c_record.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.rs_group_fma2c_train.argtypes = [vp, i32, vp, i32]
    if hasattr(L, 'rs_default_block'):      # (the host emulation of the CPU tests exports only what it implements)
        L.rs_default_block.argtypes = [i32, i32, i32]
        L.rs_default_block.restype = i32
    return L


def load_library():
    """Load libresco_sim.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('HIP extension %s is missing: build it with `python -m resco_amd.build` '
                           '(there is no CPU fallback)' % LIB_PATH)
    # PyTorch ships its own copy of the HIP runtime: when it is going to be used in this process (device tensors over the
    # library's buffers, torch.distributed), it has to be the one that is loaded first -- a process that initialises
    # /opt/rocm's runtime through this library and torch's afterwards ends up with "No HIP GPUs are available" in torch.
    if os.environ.get('RESCO_NO_TORCH') != '1':
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


AGENT = {'none': 0, 'random': 1, 'maxwave': 2, 'maxpressure': 3, 'idqn': 4, 'mplight': 5, 'ippo': 6, 'fma2c': 7}      # enum rs_agent


class Fma2cLearnConfig(C.Structure):
    """ctypes mirror of rs_fma2c_learn_config (include/resco_sim.h)"""
    _fields_ = [(k, C.c_double) for k in ('gamma', 'lr', 'alpha', 'eps', 'max_grad_norm', 'value_coef', 'entropy_coef', 'reward_norm',
                                          'reward_clip')] + [('workspace_bytes', C.c_int64)]


class GroupAgent(C.Structure):
    """ctypes mirror of rs_group_agent (include/resco_sim.h)"""
    _fields_ = [('kind', C.c_int32), ('step_key', C.c_uint32), ('policy', C.c_void_p), ('mode', C.c_int32),
                ('epsilon', C.c_float), ('epsilon_step', C.c_float), ('seed', C.c_uint32)]


class Fma2cDesc(C.Structure):
    """ctypes mirror of rs_fma2c_desc (include/resco_sim.h); ARRAYS: the pointer fields in header order"""
    ARRAYS = ('n_a', 'n_s', 'n_w', 'n_f', 'gather_off', 'gather_idx', 'gather_scale', 'fp_off', 'fp_src', 'mgr_off', 'mgr_src')
    _fields_ = [(k, C.c_int32) for k in ('K', 'M', 'S', 'n_obs', 'full')] + \
               [(k, C.c_float) for k in ('norm_wave', 'clip_wave', 'norm_wait', 'clip_wait')] + [(k, C.c_void_p) for k in ARRAYS]


class Fma2cRewardTable:
    """The reward matrix of rewards.fma2c / fma2c_full as rs_fma2c_reward_table (include/resco_sim.h): the CSR arrays of
    multi_signal.fma2c_reward_table uploaded to the device, agents in the learner's order (managers first).  The library does NOT
    check the contents, so they are asserted here before the upload.  `struct` is what the entry points take; the tensors live as
    long as this object."""

    def __init__(self, scenario, cfg, full=False, device=0):
        import torch
        from .multi_signal import fma2c_reward_table
        off, idx, w, n_rows = fma2c_reward_table(scenario, cfg, full)
        K = len(off) - 1
        assert n_rows == 3 * scenario.n_obs + 2 * scenario.n_signals
        assert off.dtype == np.int32 and idx.dtype == np.int32 and w.dtype == np.float32 and len(idx) == len(w) == int(off[-1])
        assert off[0] == 0 and bool((np.diff(off) >= 0).all()), 'off must be non-decreasing from 0'
        assert len(idx) == 0 or (0 <= int(idx.min()) and int(idx.max()) < n_rows), 'idx outside 0 .. n_rows - 1'
        dev = 'cuda:%d' % int(device)
        self.K, self.n_rows, self.nnz = K, int(n_rows), len(idx)
        self.off = torch.as_tensor(off, device=dev)
        self.idx = torch.as_tensor(idx if len(idx) else np.zeros(1, np.int32), device=dev)
        self.w = torch.as_tensor(w if len(w) else np.zeros(1, np.float32), device=dev)
        self.struct = Fma2cRewardTableStruct(K, self.n_rows, self.off.data_ptr(), self.idx.data_ptr(), self.w.data_ptr())


Rollout = RolloutStruct     # ctypes mirror of rs_rollout (include/resco_sim.h): the device buffers of one handle's trajectory segment


PPO_TENSORS = ('conv_w', 'conv_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'fc3_w', 'fc3_b', 'v_w', 'v_b')


class PPOTensors(C.Structure):
    """ctypes mirror of rs_ppo_tensors (include/resco_sim.h): ten device pointers in BatchedIPPO's layouts"""
    _fields_ = [(k, C.c_void_p) for k in PPO_TENSORS]


class PPOConfig(C.Structure):
    """ctypes mirror of rs_ppo_config (include/resco_sim.h)"""
    _fields_ = [(k, C.c_double) for k in ('lr', 'adam_eps', 'beta1', 'beta2', 'clip_eps', 'entropy_coef', 'value_coef', 'max_grad_norm')]


DQN_TENSORS = PPO_TENSORS[:8]


class DQNTensors(C.Structure):
    """ctypes mirror of rs_dqn_tensors (include/resco_sim.h): eight device pointers in BatchedIDQN's layouts"""
    _fields_ = [(k, C.c_void_p) for k in DQN_TENSORS]


class DQNConfig(C.Structure):
    """ctypes mirror of rs_dqn_config (include/resco_sim.h)"""
    _fields_ = [(k, C.c_double) for k in ('lr', 'adam_eps', 'beta1', 'beta2', 'gamma')]


class DQNRing(C.Structure):
    """ctypes mirror of rs_dqn_ring (include/resco_sim.h): the device arrays of a DeviceReplay and its position"""
    _fields_ = [(k, C.c_void_p) for k in ('obs', 'act', 'rew', 'done')] + [(k, C.c_int32) for k in ('capacity', 'n_envs', 'head', 'count')]


class DQNPer(C.Structure):
    """ctypes mirror of rs_dqn_per (include/resco_sim.h): the device arrays of the priorities and the options of prioritised replay"""
    _fields_ = [(k, C.c_void_p) for k in ('prio', 'ssum', 'pmax')] + [(k, C.c_int32) for k in ('capacity', 'n_envs')] + \
               [(k, C.c_double) for k in ('alpha', 'beta0', 'eps')] + [('beta_steps', C.c_int64)]


class MPLightRing(C.Structure):
    """ctypes mirror of rs_mplight_ring (include/resco_sim.h): the device arrays of an MPLightReplay and its position"""
    _fields_ = [(k, C.c_void_p) for k in ('obs', 'act', 'rew', 'done')] + \
               [(k, C.c_int32) for k in ('capacity', 'n_envs', 'n_signals', 'width', 'head', 'count')]


class MPLightPer(C.Structure):
    """ctypes mirror of rs_mplight_per (include/resco_sim.h): the device arrays of the priorities and the options of prioritised replay"""
    _fields_ = [(k, C.c_void_p) for k in ('prio', 'esum', 'ssum', 'pmax')] + [(k, C.c_int32) for k in ('capacity', 'n_envs', 'n_signals')] + \
               [(k, C.c_double) for k in ('alpha', 'beta0', 'eps')] + [('beta_steps', C.c_int64)]


class MPLightMap(C.Structure):
    """ctypes mirror of rs_mplight_map (include/resco_sim.h): one map of a multi-map MPLight learner"""
    _fields_ = [('n_pairs', C.c_int32), ('pairs', C.c_void_p), ('n_signals', C.c_int32)]


class SimGroup:
    """The handles ("pipes") of one GPU stepped together by ONE call through the C ABI per env-step (rs_group_step): for every
    pipe the agent's kernel and the step kernel on the pipe's own stream.  agent: 'none' | 'random' | 'maxwave' | 'maxpressure' |
    'idqn' | 'mplight' | 'fma2c' (policy = an rs_policy_handle: FusedIDQN.handle, FusedMPLight.handle, FusedFMA2C.handle)."""

    def __init__(self, sims):
        self.sims = list(sims)
        self._lib = self.sims[0]._lib
        self._hs = (C.c_void_p * len(self.sims))(*[s._h for s in self.sims])
        self._agent = GroupAgent()

    def step(self, agent='none', step_key=0, n_steps=1, policy=None, mode=0, epsilon=0.0, epsilon_step=0.0, seed=0):
        a = self._agent
        a.kind, a.step_key, a.policy = AGENT[agent], int(step_key) & 0xFFFFFFFF, policy
        a.mode, a.epsilon, a.epsilon_step, a.seed = int(mode), float(epsilon), float(epsilon_step), int(seed) & 0xFFFFFFFF
        if agent in ('maxwave', 'maxpressure'):
            for s in self.sims:
                s.require_output('mplight' if agent == 'maxpressure' else 'wave')
                s._ensure_maxwave_tables(1 if agent == 'maxpressure' else 0)
        if agent == 'fma2c' and not hasattr(self._lib, 'rs_fma2c_create'):
            raise RuntimeError('the loaded library has no rs_fma2c_*: rebuild it (there is no CPU fallback)')
        rc = self._lib.rs_group_step(self._hs, len(self.sims), C.byref(a), int(n_steps))
        if rc != 0:
            msgs = [m.decode() for m in (self._lib.rs_last_error(s._h) for s in self.sims) if m]
            raise RuntimeError('rs_group_step failed (%d): %s' % (rc, '; '.join(msgs)))

    def rollout(self, rollout, policy, t0=0, n_steps=1, step_key=0, seed=0):
        """rs_group_rollout: n_steps env-steps of every pipe under the IPPO actor-critic kernel (policy = FusedIPPO.handle), recorded
        into slots t0 .. t0 + n_steps - 1 of `rollout` (agents/ippo_fused.py: DeviceRollout over these sims).  Asynchronous, on the
        pipes' own streams: sync() before the segments are read."""
        a = self._agent
        a.kind, a.step_key, a.policy = AGENT['ippo'], int(step_key) & 0xFFFFFFFF, policy
        a.mode, a.epsilon, a.epsilon_step, a.seed = 0, 0.0, 0.0, int(seed) & 0xFFFFFFFF
        segs = rollout.segments(self.sims)
        rc = self._lib.rs_group_rollout(self._hs, len(self.sims), C.byref(a), segs, int(t0), int(n_steps))
        if rc != 0:
            msgs = [m.decode() for m in (self._lib.rs_last_error(s._h) for s in self.sims) if m]
            raise RuntimeError('rs_group_rollout failed (%d): %s' % (rc, '; '.join(msgs)))

    def train(self, n_steps, agent, policy, learner, ring, t0, done_step=-1, batch=32, updates_per_step=1, target_update=500, eps_start=1.0,
              eps_end=0.0, decay_steps=0, policy_seed=0, learner_seed=0, ret=None, loss_out=None):
        """rs_group_train: n_steps iterations of the --device-update training loop (record, act, step, record on every pipe's own
        stream; target sync, updates and the IDQN re-pack on the legacy default stream), enqueued by one call.  agent: 'idqn' | 'mplight';
        policy / learner: the library handles (FusedIDQN.handle / FusedMPLight.handle; the fused learner's); ring: a DQNRing or an
        MPLightRing at the position BEFORE the call; ret / loss_out: device pointers or None.  Nothing is advanced on the Python side:
        agents/train_fused.py: DeviceTrainer does that."""
        if not hasattr(self._lib, 'rs_group_train'):
            raise RuntimeError('the loaded library has no rs_group_train: rebuild it (there is no CPU fallback)')
        t = TrainStruct(AGENT[agent], ring.n_envs, policy, learner, ring.obs, ring.act, ring.rew, ring.done, ret, loss_out, int(t0), float(eps_start),
                        float(eps_end), ring.capacity, ring.head, ring.count, int(done_step), int(batch), int(updates_per_step), int(target_update),
                        int(decay_steps), int(policy_seed) & 0xFFFFFFFF, int(learner_seed) & 0xFFFFFFFF)
        rc = self._lib.rs_group_train(self._hs, len(self.sims), C.byref(t), int(n_steps))
        if rc != 0:
            msgs = [m.decode() for m in [self._lib.rs_last_error(s._h) for s in self.sims] + [self._lib.rs_last_error(None)] if m]
            raise RuntimeError('rs_group_train failed (%d): %s' % (rc, '; '.join(dict.fromkeys(msgs))))

    def ppo_train(self, n_steps, policy, learner, seg, done, last_value, adv, ret, gae_scratch, perm, t0, update0, slot0, done_step=-1, epochs=4,
                  minibatch=256, gamma=0.99, lambd=0.95, policy_seed=0, learner_seed=0, loss_out=None):
        """rs_group_ppo_train: n_steps iterations of the --device-update loop of tools/ippo_train.py (recorded env-steps; after the
        step that fills the segment's last slot the bootstrap value, GAE, the shuffle, the PPO update and the actor-critic re-pack),
        all on the legacy default stream, enqueued by one call.  A group of ONE handle.  policy / learner: the library handles
        (FusedIPPO.handle, the FusedPPOLearner's); seg: the handle's Rollout; the others: device pointers; the position (t0, update0,
        slot0) BEFORE the call.  Nothing is advanced on the Python side: agents/train_fused.py: DevicePPOTrainer does that."""
        if not hasattr(self._lib, 'rs_group_ppo_train'):
            raise RuntimeError('the loaded library has no rs_group_ppo_train: rebuild it (there is no CPU fallback)')
        t = PPOTrainStruct(policy, learner, seg, done, last_value, adv, ret, gae_scratch, perm, loss_out, int(t0), int(update0), int(slot0),
                           int(done_step), int(epochs), int(minibatch), float(gamma), float(lambd), int(policy_seed) & 0xFFFFFFFF,
                           int(learner_seed) & 0xFFFFFFFF)
        rc = self._lib.rs_group_ppo_train(self._hs, len(self.sims), C.byref(t), int(n_steps))
        if rc != 0:
            msgs = [m.decode() for m in [self._lib.rs_last_error(s._h) for s in self.sims] + [self._lib.rs_last_error(None)] if m]
            raise RuntimeError('rs_group_ppo_train failed (%d): %s' % (rc, '; '.join(dict.fromkeys(msgs))))

    def fma2c_train(self, n_steps, policy, learner, table, rows, acts, rews, vals, dones, R_boot, T, t0, slot0, done_step=-1, policy_seed=0,
                    ret=None, loss_out=None):
        """rs_group_fma2c_train: n_steps iterations of the --device-update loop of tools/fma2c_train.py (act into the segment's slot,
        step, reward and recorder; at a full segment or the episode's end the bootstrap value and the A2C update), all on the legacy
        default stream, enqueued by one call.  A group of ONE handle.  policy / learner: the library handles (FusedFMA2C.handle, the
        FusedA2CLearner's); table: an Fma2cRewardTable; the others: device pointers of the learner's segment; the position (t0,
        slot0) BEFORE the call.  Nothing is advanced on the Python side: agents/train_fused.py: DeviceA2CTrainer does that."""
        if not hasattr(self._lib, 'rs_group_fma2c_train'):
            raise RuntimeError('the loaded library has no rs_group_fma2c_train: rebuild it (there is no CPU fallback)')
        t = Fma2cTrainStruct(policy, learner, table.struct if hasattr(table, 'struct') else table, rows, acts, rews, vals, dones, R_boot, ret,
                             loss_out, int(t0), int(T), int(slot0), int(done_step), int(policy_seed) & 0xFFFFFFFF)
        rc = self._lib.rs_group_fma2c_train(self._hs, len(self.sims), C.byref(t), int(n_steps))
        if rc != 0:
            msgs = [m.decode() for m in [self._lib.rs_last_error(s._h) for s in self.sims] + [self._lib.rs_last_error(None)] if m]
            raise RuntimeError('rs_group_fma2c_train failed (%d): %s' % (rc, '; '.join(dict.fromkeys(msgs))))

    def sync(self):
        for s in self.sims:
            s.sync()


def _murmur(seed, words):
    """the counter-based hash of the model (resco_amd/csrc/resco_step.h: d_hash) on the host"""
    M = 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M
    h = seed & M
    for k in words:
        k = (k * 0xcc9e2d51) & M
        k = rotl(k, 15)
        k = (k * 0x1b873593) & M
        h ^= k
        h = rotl(h, 13)
        h = (h * 5 + 0xe6546b64) & M
    h ^= 16
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M
    h ^= h >> 16
    return h


def speed_factor(seed, env, trip, vt_row, speed_dev=1):
    """speedFactor of a trip (resco_step.h: speed_factor): a function of (seed, global env index, trip) only, so it can be
    recomputed for trips that have left the network (tripinfo output)"""
    mean, dev = np.float32(vt_row[7]), np.float32(vt_row[8])
    f = mean
    if speed_dev:
        s = np.float32(0.0)
        for i in range(4):
            s = np.float32(s + np.float32(_murmur(seed, (env, trip, 0xFFFFFFFF, i)) >> 8) * np.float32(1.0 / 16777216.0))
        z = np.float32((s - np.float32(2.0)) * np.float32(1.7320508))
        f = np.float32(mean + np.float32(dev * z))
    f = min(max(np.float32(f), np.float32(0.2)), np.float32(2.0))
    return float(np.float32(int(np.float32(f * np.float32(4096.0)) + np.float32(0.5))) * np.float32(1.0 / 4096.0))     # RM_SF_QUANT


def torch_stream(device=None):
    """The stream argument that orders a launch with PyTorch's current stream.  PyTorch's default stream has the
    handle 0, which the C ABI reads as "the handle's own stream": it is mapped to hipStreamLegacy (1)."""
    import torch
    p = torch.cuda.current_stream(device).cuda_stream
    return p if p else 1


class _DevArray:
    """Zero-copy view of a library-owned device buffer (__cuda_array_interface__, also honoured on ROCm)."""

    def __init__(self, ptr, shape, dtype_code, owner):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=_TYPESTR[dtype_code],
                                             data=(int(ptr), False), version=2, strides=None)
        self._owner = owner


class BatchedSim:
    """N lock-step environments of one scenario on one GPU (one rs_handle)."""

    def __init__(self, scenario, n_envs, device=0, seed=0, max_distance=200.0, sigma=-1.0, speed_dev=1,
                 fixed_program=0, env_base=0, step_length=10, yellow_length=None, block_threads=0, trip_log=0, step_ratio=1,
                 tls_expiry=1, device_envs=None):
        """device_envs: how many environments share this GPU when the batch is split over several handles (pipes) -- the default
        workgroup shape (block_threads = 0) is chosen for the device's load, not for this handle's share (rs_default_block)"""
        self.sc = scenario
        self.n_envs = int(n_envs)
        self.device = int(device)
        self._lib = self._load()
        if yellow_length is not None and int(yellow_length) != int(scenario.yellow_length):
            # the yellow phases are compiled into the scenario's programmes with ITS yellow_length; the FSM would call
            # set_phase after a different number of ticks
            raise ValueError('scenario %s was compiled with yellow_length=%d (asked %d)' % (scenario.name, scenario.yellow_length, yellow_length))
        self._st, self._keep = pack_scenario(scenario, step_length, yellow_length)
        self._p = ParamsStruct(int(seed) & 0xFFFFFFFF, float(max_distance), float(sigma), int(speed_dev),
                               int(fixed_program), int(trip_log), int(step_ratio), 0 if tls_expiry else 1)     # rs_params.tls_hold
        self.step_ratio = max(1, int(step_ratio))
        self._h = C.c_void_p()
        if not block_threads and device_envs and int(device_envs) != self.n_envs and hasattr(self._lib, 'rs_default_block'):
            block_threads = self._lib.rs_default_block(int(scenario.capacity), int(device_envs), self.device)
        rc = self._lib.rs_create(C.byref(self._st), C.byref(self._p), self.n_envs, int(env_base), self.device,
                                 int(block_threads), C.byref(self._h))
        if rc != 0:
            msg = self._lib.rs_last_error(None)
            self._h = None
            raise RuntimeError('rs_create failed (%d): %s' % (rc, msg.decode() if msg else '?'))
        self.S, self.O, self.C = scenario.n_signals, scenario.n_obs, scenario.capacity
        self.seed, self.env_base, self.speed_dev = int(seed) & 0xFFFFFFFF, int(env_base), int(speed_dev)
        self._maxwave_ready = False
        self._masked_off = frozenset()          # maskable output buffers the observe does not write at present (set_outputs)
        self._dep_cache = None
        self._demand = None                     # the variants in force (set_demand): (scenarios, env_variant)
        self._meta = {}
        for name, bid in BUF_ID.items():
            ptr, shape, nd, dt = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(), C.c_int32()
            self._check(self._lib.rs_get_buffer(self._h, bid, C.byref(ptr), shape, C.byref(nd), C.byref(dt)))
            self._meta[name] = (ptr.value, tuple(shape[:nd.value]), dt.value)

    # ------------------------------------------------------------------ plumbing
    def _load(self):
        return load_library()

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.rs_last_error(self._h)
            raise RuntimeError('resco_sim error %d: %s' % (rc, msg.decode() if msg else '?'))

    def close(self):
        if getattr(self, '_h', None):
            self._lib.rs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.rs_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        out = dict(n_envs=a.value, block_threads=b.value, lds_bytes=c.value, max_lanes_per_signal=d.value)
        if hasattr(self._lib, 'rs_info_kernel'):      # (a library built before the per-map step kernels has no such entry)
            out['step_kernel'] = self._lib.rs_info_kernel(self._h).decode()
        return out

    # ------------------------------------------------------------------ stepping
    def reset(self, stream=None):
        self._check(self._lib.rs_reset(self._h, stream))

    def step(self, actions=None, stream=None):
        """actions: None (use the on-device action buffer), a numpy int32 [N,S] array, or a torch
        CUDA int32 tensor [N,S]."""
        if actions is None:
            self._check(self._lib.rs_step(self._h, None, 0, stream))
            return
        if hasattr(actions, 'data_ptr'):        # torch tensor
            assert tuple(actions.shape) == (self.n_envs, self.S) and actions.is_contiguous()
            assert str(actions.dtype) == 'torch.int32'
            self._check(self._lib.rs_step(self._h, actions.data_ptr(), 1 if actions.is_cuda else 0, stream))
            return
        a = np.ascontiguousarray(actions, dtype=np.int32)
        assert a.shape == (self.n_envs, self.S), a.shape
        self._check(self._lib.rs_step(self._h, a.ctypes.data, 0, stream))

    def ticks(self, n, stream=None):
        """n x step_sim() without the signal FSM, then an observe (see rs_ticks)"""
        self._check(self._lib.rs_ticks(self._h, int(n), stream))

    def step_sim(self, n=1, stream=None):
        """n x sumo.simulationStep() and nothing else: no observe, the Signal state stays as it is (see rs_step_sim)"""
        self._check(self._lib.rs_step_sim(self._h, int(n), stream))

    def set_outputs(self, names=None):
        """Only the named per-lane / per-movement buffers ('lane_agg', 'drq_norm', 'drq_norm_f16', 'lane_arrivals', 'mplight',
        'wave', 'mplight_full') are written by the following observes; None = all of them.  The per-signal scalars (phase,
        wait, wait_norm, pressure, queue_sum, queue_max, arrivals, departures) are always written (see rs_set_outputs)."""
        mask = 0
        for n in (OUTPUT_GROUPS if names is None else names):
            if n not in OUTPUT_GROUPS:
                raise ValueError('%r is not a maskable output buffer (%s)' % (n, ', '.join(OUTPUT_GROUPS)))
            mask |= 1 << BUF_ID[n]
        self._check(self._lib.rs_set_outputs(self._h, mask))
        self._masked_off = frozenset(OUTPUT_GROUPS) - frozenset(OUTPUT_GROUPS if names is None else names)

    def require_output(self, name):
        """Raise when `name` is a maskable output buffer that set_outputs has switched off: its contents are stale (or zeros),
        and whoever consumes them (an on-device agent, a derived state) would act on garbage without noticing."""
        if name in self._masked_off:
            raise RuntimeError('output buffer %r is switched off (BatchedSim.set_outputs): re-enable it before reading it' % name)

    def reinit_signals(self, stream=None):
        """fresh Signal objects on the running simulation (see rs_reinit_signals)"""
        self._check(self._lib.rs_reinit_signals(self._h, stream))

    def set_seed(self, seed):
        self.seed = int(seed) & 0xFFFFFFFF
        self._check(self._lib.rs_set_seed(self._h, self.seed))

    def sync(self):
        self._check(self._lib.rs_sync(self._h))

    # ------------------------------------------------------------------ per-environment demand
    def set_demand(self, scenarios, env_variant=None):
        """Every environment runs the trips of its own demand variant from the NEXT reset() on (rs_set_demand): call it right before
        reset(), as set_seed.  scenarios: K Scenarios that differ from this handle's in their trips alone (demand.with_trips,
        demand.demand_variant, demand.demand_set); env_variant: int [n_envs] in 0 .. K - 1, default (env_base + e) % K
        (demand.env_variants).  The host-side figures (backlog, trip_metrics, ...) follow each environment's variant.  An empty list
        is clear_demand()."""
        from .demand import env_variants
        if not hasattr(self._lib, 'rs_set_demand'):
            raise RuntimeError('the loaded library has no rs_set_demand: rebuild it (there is no CPU fallback)')
        scenarios = list(scenarios)
        K = len(scenarios)
        if K == 0:
            return self.clear_demand()
        A = self.sc.arrays
        for k, v in enumerate(scenarios):
            if v.n_trips != self.sc.n_trips:
                raise ValueError('demand variant %d has %d trips, the scenario %d (demand.with_trips keeps the number)' % (k, v.n_trips, self.sc.n_trips))
            if v.n_routes != self.sc.n_routes or not np.array_equal(v.arrays['route_edge'], A['route_edge']) or v.horizon != self.sc.horizon:
                raise ValueError('demand variant %d is not a variant of this scenario (other routes or horizon)' % k)
        ev = env_variants(self.n_envs, self.env_base, K) if env_variant is None else np.ascontiguousarray(env_variant, dtype=np.int32)
        if ev.shape != (self.n_envs,):
            raise ValueError('env_variant must have one entry per environment (%d), got shape %s' % (self.n_envs, ev.shape))
        structs, keep = (DemandStruct * K)(), []
        for k, v in enumerate(scenarios):
            for name in ('trip_depart', 'trip_route', 'trip_vtype'):
                a = np.ascontiguousarray(v.arrays[name], dtype=np.int32)
                keep.append(a)
                setattr(structs[k], name, a.ctypes.data_as(C.POINTER(C.c_int32)))
        self._check(self._lib.rs_set_demand(self._h, K, structs, ev.ctypes.data))
        del keep
        self._demand = (scenarios, ev.copy())
        self._dep_cache = None

    def clear_demand(self):
        """back to the scenario's own trips in every environment, from the next reset() on; nothing happens (no call, no new demand
        generation: earlier snapshots stay valid) when no variants are in force"""
        if self._demand is None:
            return
        self._check(self._lib.rs_set_demand(self._h, 0, None, None))
        self._demand = None
        self._dep_cache = None

    def demand_info(self):
        """(K, env_variant) as the library holds them; (0, None) without variants"""
        if not hasattr(self._lib, 'rs_demand_info'):
            return 0, None
        k, ev = C.c_int32(), np.zeros(self.n_envs, np.int32)
        self._check(self._lib.rs_demand_info(self._h, C.byref(k), ev.ctypes.data))
        return k.value, (ev if k.value else None)

    def env_scenarios(self):
        """the scenario whose trips each environment runs: [n_envs] (its variant's, or the handle's own)"""
        if self._demand is None:
            return [self.sc] * self.n_envs
        scenarios, ev = self._demand
        return [scenarios[int(k)] for k in ev]

    def _demand_groups(self):
        """[(scenario, environments that run its trips)]: one group per variant in use, or the handle's scenario and everyone"""
        if self._demand is None:
            return [(self.sc, np.arange(self.n_envs))]
        scenarios, ev = self._demand
        return [(scenarios[k], np.nonzero(ev == k)[0]) for k in range(len(scenarios)) if bool((ev == k).any())]

    def scheduled(self):
        """the demand of every environment: the trips of its variant with depart <= horizon (padding trips are not demand)"""
        out = np.zeros(self.n_envs, np.int64)
        for sc, envs in self._demand_groups():
            out[envs] = int((sc.arrays['trip_depart'] <= sc.horizon).sum())
        return out

    def fma2c_record(self, policy, table, rew_out, acts_out=None, ret_acc=None, stream=None):
        """rs_fma2c_record: the FMA2C rewards of all agents (RAW) into rew_out f32 [N, K]; acts_out int32 [N, K] = the managers' and
        the workers' actions of the step; ret_acc f32 [N, K] += the reward.  policy: an rs_policy_handle (FusedFMA2C.handle); table:
        an Fma2cRewardTable (or None, which the library refuses); the others: device tensors or None."""
        if not hasattr(self._lib, 'rs_fma2c_record'):
            raise RuntimeError('the loaded library has no rs_fma2c_record: rebuild it (there is no CPU fallback)')
        ptr = lambda t: t.data_ptr() if t is not None else None
        tab = C.byref(table.struct) if hasattr(table, 'struct') else (C.byref(table) if table is not None else None)
        rc = self._lib.rs_fma2c_record(self._h, policy, tab, ptr(rew_out), ptr(acts_out), ptr(ret_acc), stream)
        if rc != 0:
            raise RuntimeError('rs_fma2c_record failed (%d): %s' % (rc, (self._lib.rs_last_error(self._h) or b'?').decode()))

    def act_random(self, step_key, stream=None):
        self._check(self._lib.rs_act_random(self._h, int(step_key) & 0xFFFFFFFF, stream))

    def act_maxwave(self, use_pressure, stream=None):
        if not self._maxwave_ready:
            pairs, valid, order = maxwave_tables(self.sc)
            self._pairs, self._valid, self._order = pairs, valid, order
            self._check(self._lib.rs_act_maxwave(self._h, pairs.ctypes.data, len(pairs), valid.ctypes.data,
                                                 order.ctypes.data, int(use_pressure), stream))
            self._maxwave_ready = True
            return
        self._check(self._lib.rs_act_maxwave(self._h, None, len(self._pairs), None, None, int(use_pressure), stream))

    def _ensure_maxwave_tables(self, use_pressure):
        """the phase-pair tables live on the device after the first rs_act_maxwave call (rs_group_step needs them there)"""
        if not self._maxwave_ready:
            self.act_maxwave(use_pressure)

    # ------------------------------------------------------------------ buffers
    def read(self, name):
        """Synchronous host copy of a buffer as a numpy array."""
        ptr, shape, dt = self._meta[name]
        out = np.empty(shape, _NP_DTYPES[dt])
        if out.nbytes == 0:
            return out
        self._check(self._lib.rs_read_buffer(self._h, BUF_ID[name], out.ctypes.data, out.nbytes))
        return out

    def tensor(self, name, allow_masked=False):
        """Zero-copy torch tensor over the library-owned device buffer (agent boundary).  A buffer that set_outputs has
        switched off is refused (stale contents) unless allow_masked."""
        import torch
        if not allow_masked:
            self.require_output(name)
        ptr, shape, dt = self._meta[name]
        return torch.as_tensor(_DevArray(ptr, shape, dt, self), device='cuda:%d' % self.device)

    def device_pointer(self, name):
        return self._meta[name]

    def outputs(self, names=('lane_agg', 'drq_norm', 'phase', 'mplight', 'wave', 'wait', 'wait_norm', 'pressure',
                             'queue_sum', 'queue_max')):
        return {n: self.read(n) for n in names}

    def stats(self):
        st = self.read('stats')
        return {k: st[:, i].copy() for i, k in enumerate(STAT_KEYS)}

    def time(self):
        return self.read('env')[:, 0]

    def _dep_lanes(self, sc=None):
        """The departure lanes in the kernel's numbering (resco_tables.h: the first allowed lane of the first edge of every
        ROUTE, ascending) and, per lane, its trips in FIFO order with their departure seconds and running sums -- of the handle's
        scenario or of a demand variant (the lanes are the same: they come from the routes; a lane may have no trip)."""
        sc = self.sc if sc is None else sc
        if self._dep_cache is None:
            self._dep_cache = {}
        if id(sc) not in self._dep_cache:
            A = sc.arrays
            lane_of_route = A['edge_lane0'][A['route_edge'][A['route_start'][:-1]]]
            lanes = np.unique(lane_of_route)
            n_dep = self._meta['dep_next'][1][1]
            if len(lanes) != n_dep:
                raise RuntimeError('departure lanes of the scenario (%d) do not match the library (%d)' % (len(lanes), n_dep))
            lane_of_trip = lane_of_route[A['trip_route']]
            depart = A['trip_depart'].astype(np.int64)
            tabs = []
            for lane in lanes:
                trips = np.nonzero(lane_of_trip == lane)[0]          # ascending trip index = FIFO order = departure order
                dep = depart[trips]
                tabs.append((trips, dep, np.concatenate([[0], np.cumsum(dep)])))
            self._dep_cache[id(sc)] = (sc, tabs)                     # (the scenario is held: its id stays its own)
        return self._dep_cache[id(sc)][1]

    def backlog(self):
        """Trips that have departed (depart < now) but are not on the network yet, per environment: (count, seconds
        waited so far).  Every departure lane keeps its own backlog (RS_BUF_DEP_NEXT = its next trip); utils/readXML.py:52-68
        charges such trips end_time - depart."""
        head = self.read('dep_next').astype(np.int64)            # [N, n_dep]
        now = self.time().astype(np.int64)
        cnt = np.zeros(self.n_envs, np.int64)
        waited = np.zeros(self.n_envs, np.int64)
        for sc, envs in self._demand_groups():           # every environment against the trips of its own demand variant
            for d, (trips, dep, csum) in enumerate(self._dep_lanes(sc)):
                h, t = head[envs, d], now[envs]
                first = np.where(h == TRIP_NONE, len(trips), np.searchsorted(trips, h))
                due = np.searchsorted(dep, t, side='left')
                if self._demand is not None:        # (a trip of a VARIANT scheduled beyond the horizon is padding, not demand; a handle without variants counts as ever)
                    due = np.minimum(due, np.searchsorted(dep, sc.horizon, side='right'))
                last = np.maximum(first, due)                                     # trips [first, last) are due and waiting
                cnt[envs] += last - first
                waited[envs] += (last - first) * t - (csum[last] - csum[first])
        return cnt, waited

    def trip_delay(self):
        """Per-environment average trip delay exactly as the reference's post-processing computes it, see trip_metrics()."""
        return self.trip_metrics()['delay']

    def trip_metrics(self):
        """The per-episode figures of utils/readXML.py:16-77 per environment.
        `delay`: (timeLoss + departDelay) summed over the tripinfo entries -- the arrived and, as
        --tripinfo-output.write-unfinished writes them, the running vehicles -- divided by their number.  Demand that never got
        onto the network is added only when the rou.xml lists <vehicle> elements (cologne3): readXML.py:59-68 skips every other
        tag, so the <trip> files of five of the six maps are never charged for it.  For <vehicle> files the script's own rule is
        followed (`_readxml_never_departed`): every vehicle SCHEDULED later than the vehicle that actually departed last counts as
        never departed and is charged end_time - depart -- whether or not it is in the tripinfo file as well.
        `delay_all` charges the insertion backlogs (trips that are due and not on the network, now - depart each) on every map:
        this build's own, stricter figure, not the script's.  `duration`, `waiting`, `time_loss`: tripinfo duration /
        waitingTime / timeLoss over the same entries."""
        st = self.stats()
        lane = self.read('veh_lane')
        live = lane != 0xFFFF
        running = (self.read('veh_tloss') * live).sum(axis=1)
        cnt, waited = self.backlog()
        now = self.time().astype(np.int64)
        entries = st['arrived'] + live.sum(axis=1)
        depart = self.read('veh_depart').astype(np.int64)
        run_dur = ((now[:, None] - depart) * live).sum(axis=1)
        loss = st['sum_time_loss_q10'] / 1024.0 + running
        delay_all = (loss + st['sum_depart_delay'] + waited) / np.maximum(1, entries + cnt)
        if self.sc.demand_tag == 'vehicle':
            n_nd, charged = self._readxml_never_departed(live, depart)
            delay = (loss + st['sum_depart_delay'] + charged) / np.maximum(1, entries + n_nd)
        else:
            delay = (loss + st['sum_depart_delay']) / np.maximum(1, entries)
        entries = np.maximum(1, entries)
        return dict(delay=delay, delay_all=delay_all, duration=(st['sum_duration'] + run_dur) / entries,
                    waiting=st['sum_waiting'] / entries, time_loss=loss / entries)

    def _readxml_never_departed(self, live, depart):
        """utils/readXML.py:41-68 for <vehicle> route files, per environment: (count, seconds charged).  The script takes the
        tripinfo entry with the latest actual departure (the first one in file order among equals: arrived vehicles come first,
        in arrival order; the unfinished ones follow in id order), looks up that vehicle's SCHEDULED departure in the rou.xml and
        charges end_time - depart for every <vehicle> scheduled later.  Arrived vehicles are considered when the handle keeps
        per-trip records (trip_log=1); without them the latest departure is taken from the vehicles still on the network."""
        horizon = int(self.sc.horizon)
        trips = self.read('veh_trip').astype(np.int64)
        env_sc = self.env_scenarios()           # the schedule and the ids of every environment's own demand variant
        log = self.read('trip_log') if self._p.trip_log else None
        n_nd = np.zeros(self.n_envs, np.int64)
        charged = np.zeros(self.n_envs, np.float64)
        for e in range(self.n_envs):
            sched = env_sc[e].arrays['trip_depart'].astype(np.int64)
            ids = getattr(env_sc[e], 'trip_ids', None)
            best_t, best_k = -1, -1
            if log is not None and log.size:
                arr = np.nonzero(log[e, :, 1] > 0)[0]
                if len(arr):
                    t = log[e, arr, 0]
                    order = np.lexsort((arr, log[e, arr, 1]))           # file order: arrival time, then trip order
                    j = order[np.argmax(t[order] == t.max())]
                    best_t, best_k = int(t[j]), int(arr[j])
            run = np.nonzero(live[e])[0]
            if len(run):
                t = depart[e, run]
                if int(t.max()) > best_t:
                    cand = trips[e, run[t == t.max()]]
                    best_k = int(min(cand, key=(lambda k: ids[k]) if ids else None))
                    best_t = int(t.max())
            if best_k < 0:
                continue
            late = sched > sched[best_k]
            if self._demand is not None:
                late &= sched <= horizon        # (beyond the horizon: padding of a demand variant, charged nowhere)
            n_nd[e] = int(late.sum())
            charged[e] = float((horizon - sched[late]).sum())
        return n_nd, charged

    # ------------------------------------------------------------------ snapshots / timing
    def snapshot(self):
        snap = C.c_void_p()
        self._check(self._lib.rs_snapshot(self._h, C.byref(snap)))
        return snap

    def restore(self, snap):
        self._check(self._lib.rs_restore(self._h, snap))

    def free_snapshot(self, snap):
        self._lib.rs_snapshot_free(self._h, snap)

    def phase_profile(self, enable):
        """Enable/disable the in-kernel phase timers; returns the 16 accumulators collected so far."""
        out = (C.c_uint64 * 16)()
        self._check(self._lib.rs_phase_profile(self._h, 1 if enable else 0, out))
        return [int(x) for x in out]

    def timing(self, enable):
        self._check(self._lib.rs_timing(self._h, 1 if enable else 0))

    def timing_read(self):
        ms, n = C.c_float(), C.c_int32()
        self._check(self._lib.rs_timing_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def maxwave_tables(sc):
    """phase_pairs [P][2], valid [S][P] (local action of pair p or -1) and order [S][P] (pair indices in
    the reference's iteration order, -1 padded) for the batched MAXWAVE / MAXPRESSURE agent
    (agents/maxwave.py:18-38).  Without valid_acts every pair k maps to action k (np.argmax branch)."""
    pairs = np.asarray(sc.phase_pairs, np.int32).reshape(-1, 2)
    S, P = sc.n_signals, len(pairs)
    valid = np.full((S, P), -1, np.int32)
    order = np.full((S, P), -1, np.int32)
    for si, sid in enumerate(sc.signal_ids):
        va = None if sc.valid_acts is None else sc.valid_acts.get(sid)
        if va is None:
            valid[si, :] = np.arange(P)
            order[si, :] = np.arange(P)
        else:
            for j, (gidx, act) in enumerate(va.items()):        # dict order = the reference's iteration order
                valid[si, int(gidx)] = int(act)
                order[si, j] = int(gidx)
    return np.ascontiguousarray(pairs), np.ascontiguousarray(valid), np.ascontiguousarray(order)
