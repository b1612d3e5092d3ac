"""BasicCollector: the reference's single-env collector surface (fsrl/data/basic_collector.py) over FastCollector.

`BasicCollector(policy, env, traj_buffer=TrajectoryBuffer(100)).collect(n_episode)` works as in the reference.  A single env is
wrapped into a vector env of one (as_vector_env), a vector env is taken as it is.  The reference's collector hands every transition
to `traj_buffer.store`; here the trajectory buffer taps the store ingest of the policy's engine (TrajectoryBuffer.attach), so the
rows have to go through that store: without a `buffer` the collector makes the engine's HipVectorReplayBuffer its own."""
from fsrl_amd.data.fast_collector import FastCollector


class BasicCollector(FastCollector):
    def __init__(self, policy, env, buffer=None, exploration_noise: bool = False, traj_buffer=None, **fast_collector_options):
        engine = getattr(policy, "engine", None)
        if traj_buffer is not None and engine is None:
            raise TypeError("BasicCollector(traj_buffer=...): the trajectory buffer records what goes through an Engine's store; "
                            "this policy has no engine")
        if buffer is None and engine is not None:
            from fsrl_amd.data.buffer import HipVectorReplayBuffer
            buffer = HipVectorReplayBuffer(engine)
        super().__init__(policy, env, buffer, exploration_noise=exploration_noise, **fast_collector_options)
        if traj_buffer is not None:
            traj_buffer.attach(self)
