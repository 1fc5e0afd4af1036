"""agent_configs (same keys as resco_benchmark/config/agent_config.py:65-82, 101-113, 141-153): which state / reward functions
and detector range each agent is run with, and MPLight's hyper-parameters (resco_amd/agents/mplight.py).  IDQN and IPPO are
driven by their own batched modules (resco_amd/agents/idqn_*.py, ippo.py; tools/idqn_train.py, ippo_train.py).  FMA2C, FMA2CFULL
and FMA2CVAL carry the reference's hyper-parameters (agent_config.py:39-63, 114-138, 154-178) for resco_amd/agents/fma2c.py; the
batched path is tools/fma2c_train.py."""
from .. import rewards, states
from ..agents.fma2c import FMA2C
from ..agents.mplight import MPLight
from ..agents.static_agents import MAXPRESSURE, MAXWAVE, STOCHASTIC

_FMA2C = {'agent': FMA2C, 'management_acts': 4, 'rmsp_alpha': 0.99, 'rmsp_epsilon': 1e-5, 'max_grad_norm': 40, 'gamma': 0.96,
          'lr_init': 2.5e-4, 'lr_decay': 'constant', 'entropy_coef_init': 0.001, 'entropy_coef_min': 0.001, 'entropy_decay': 'constant',
          'entropy_ratio': 0.5, 'value_coef': 0.5, 'num_lstm': 64, 'num_fw': 128, 'num_ft': 32, 'num_fp': 64, 'batch_size': 120,
          'reward_norm': 2000.0, 'reward_clip': 2.0}

agent_configs = {
    'STOCHASTIC': {'agent': STOCHASTIC, 'state': states.mplight, 'reward': rewards.wait, 'max_distance': 1},
    'MAXWAVE': {'agent': MAXWAVE, 'state': states.wave, 'reward': rewards.wait, 'max_distance': 50},
    'MAXPRESSURE': {'agent': MAXPRESSURE, 'state': states.mplight, 'reward': rewards.wait, 'max_distance': 200},
    'MAXWAVEVAL': {'agent': MAXWAVE, 'state': states.wave, 'reward': rewards.wait, 'max_distance': 50},
    'MAXPRESSUREVAL': {'agent': MAXPRESSURE, 'state': states.mplight, 'reward': rewards.wait,
                       'max_distance': 9999},
    'MPLight': {'agent': MPLight, 'state': states.mplight, 'reward': rewards.pressure, 'max_distance': 200, 'BATCH_SIZE': 32,
                'GAMMA': 0.99, 'EPS_START': 1.0, 'EPS_END': 0.0, 'EPS_DECAY': 220, 'TARGET_UPDATE': 500, 'demand_shape': 1},
    # *FULL: the state extended by what IDQN observes
    'MPLightFULL': {'agent': MPLight, 'state': states.mplight_full, 'reward': rewards.pressure, 'max_distance': 200, 'BATCH_SIZE': 32,
                    'GAMMA': 0.99, 'EPS_START': 1.0, 'EPS_END': 0.0, 'EPS_DECAY': 220, 'TARGET_UPDATE': 500, 'demand_shape': 4},
    'FMA2C': dict(_FMA2C, state=states.fma2c, reward=rewards.fma2c, max_distance=200),
    'FMA2CFULL': dict(_FMA2C, state=states.fma2c_full, reward=rewards.fma2c_full, max_distance=200),
    'FMA2CVAL': dict(_FMA2C, state=states.fma2c, reward=rewards.fma2c, max_distance=50),
}
