"""drl-dronenavigation_amd -- MI355X-native vectorised drone-navigation RL environment.

The hot path of eRGiBi/DRL-DroneNavigation (PBDroneEnv.step -> BaseAviary.step -> PyBullet,
behind SB3's SubprocVecEnv) as hand-written HIP kernels for gfx950 behind a C ABI
(include/dronenav.h, csrc/), plus the thin Python host mirror of the reference's VecEnv surface.
Importing this package needs the compiled library (there is no CPU fallback); build it with
`python __graft_entry__.py` or `drl-dronenavigation_amd/build.py`.
"""
from . import _capi, build, tracks  # noqa: F401
from ._capi import DroneNavError, DroneNavLibraryError  # noqa: F401
from .tracks import Track, TrackBank  # noqa: F401
from .dynamics import DynamicsRandomization  # noqa: F401
from .wind import WindDisturbance  # noqa: F401
from .actuator import ActuatorModel  # noqa: F401
from .sensor import SensorModel  # noqa: F401
from .privileged import PrivilegedObservation, PRIV_DIM, PRIV_GROUPS, PRIV_SLICES  # noqa: F401
from .goal import GoalObservation, GOAL_DIM, GOAL_FRAMES, GOAL_SLICES  # noqa: F401
from .history import HistoryObservation  # noqa: F401

__all__ = ["DroneVecEnv", "Track", "TrackBank", "tracks", "gae", "DroneNavError", "DroneNavLibraryError", "make_config",
           "RolloutCollector", "ShardPlan", "all_gather_rollout", "preprocess_action", "stream_copy", "MlpActorCritic", "SacActor", "FusedSacActor",
           "FusedMlpPolicy", "MlpValue", "FusedMlpValue",
           "DynamicsRandomization", "WindDisturbance", "ActuatorModel", "SensorModel",
           "PrivilegedObservation", "PRIV_DIM", "PRIV_GROUPS", "PRIV_SLICES",
           "GoalObservation", "GOAL_DIM", "GOAL_FRAMES", "GOAL_SLICES", "HistoryObservation", "RowNormalizer",
           "ReturnNormalizer", "MinibatchSampler", "PpoLoss", "ClippedAdam", "MlpTrainer", "ReplaySampler", "SacPolicyHead", "SacCriticLoss", "SacActorLoss",
           "SacCritic", "SacTrainer", "PolyakUpdate", "LstmTrainer", "LstmStepper"]


def __getattr__(name):
    # vec_env imports torch; keep `import drl_dronenavigation_amd` light for tools that only build.
    import importlib
    if name in ("DroneVecEnv", "gae", "make_config", "vec_env", "preprocess_action", "stream_copy"):
        vec_env = importlib.import_module(__name__ + ".vec_env")
        return vec_env if name == "vec_env" else getattr(vec_env, name)
    if name in ("collector", "RolloutCollector", "ShardPlan", "all_gather_rollout", "ReplayBuffer", "RingReplayBuffer", "OffPolicyCollector",
                "FusedRolloutCollector"):
        collector = importlib.import_module(__name__ + ".collector")
        return collector if name == "collector" else getattr(collector, name)
    if name in ("policy_mfma", "FusedMlpPolicy", "FusedSacActor", "FusedMlpValue"):
        pm = importlib.import_module(__name__ + ".policy_mfma")
        return pm if name == "policy_mfma" else getattr(pm, name)
    if name in ("rownorm", "RowNormalizer"):
        rownorm = importlib.import_module(__name__ + ".rownorm")
        return rownorm if name == "rownorm" else rownorm.RowNormalizer
    if name in ("retnorm", "ReturnNormalizer"):
        retnorm = importlib.import_module(__name__ + ".retnorm")
        return retnorm if name == "retnorm" else retnorm.ReturnNormalizer
    if name in ("minibatch", "MinibatchSampler"):
        minibatch = importlib.import_module(__name__ + ".minibatch")
        return minibatch if name == "minibatch" else minibatch.MinibatchSampler
    if name in ("ppo", "PpoLoss"):
        ppo = importlib.import_module(__name__ + ".ppo")
        return ppo if name == "ppo" else ppo.PpoLoss
    if name in ("optim", "ClippedAdam"):
        optim = importlib.import_module(__name__ + ".optim")
        return optim if name == "optim" else optim.ClippedAdam
    if name in ("mlp_train", "MlpTrainer"):
        mlp_train = importlib.import_module(__name__ + ".mlp_train")
        return mlp_train if name == "mlp_train" else mlp_train.MlpTrainer
    if name in ("replay", "ReplaySampler"):
        replay = importlib.import_module(__name__ + ".replay")
        return replay if name == "replay" else replay.ReplaySampler
    if name in ("sac", "SacPolicyHead", "SacCriticLoss", "SacActorLoss"):
        sac = importlib.import_module(__name__ + ".sac")
        return sac if name == "sac" else getattr(sac, name)
    if name in ("sac_train", "SacTrainer", "PolyakUpdate"):
        sac_train = importlib.import_module(__name__ + ".sac_train")
        return sac_train if name == "sac_train" else getattr(sac_train, name)
    if name in ("lstm_train", "LstmTrainer", "LstmStepper"):
        lstm_train = importlib.import_module(__name__ + ".lstm_train")
        return lstm_train if name == "lstm_train" else getattr(lstm_train, name)
    if name == "metrics":
        return importlib.import_module(__name__ + ".metrics")
    if name in ("policy", "MlpActorCritic", "SacActor", "SacCritic", "MlpValue"):
        policy = importlib.import_module(__name__ + ".policy")
        return policy if name == "policy" else getattr(policy, name)
    raise AttributeError(name)
