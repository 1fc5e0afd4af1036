"""agent_configs (same keys as resco_benchmark/config/agent_config.py:65-82, 101-113, 141-153): which state / reward functions
and detector range each agent is run with, and MPLight's hyper-parameters (resco_amd/agents/mplight.py).  IDQN and IPPO are
driven by their own batched modules (resco_amd/agents/idqn_*.py, ippo.py; tools/idqn_train.py, ippo_train.py); FMA2C's learner
is out of scope."""
from .. import rewards, states
from ..agents.mplight import MPLight
from ..agents.static_agents import MAXPRESSURE, MAXWAVE, STOCHASTIC

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
}
