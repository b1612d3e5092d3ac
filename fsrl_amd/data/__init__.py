"""Host-side data plumbing: a minimal Batch, the proxy of the HIP-resident store, the collectors."""
from fsrl_amd._lazy import install

install(__name__, globals(), {
    "Batch": "batch",
    "HipVectorReplayBuffer": "buffer",
    "HipPrioritizedVectorReplayBuffer": "buffer",
    "FastCollector": "fast_collector",
    "DeviceCollector": "device_collector",
    "DeviceEvalCollector": "device_collector",
    "GroupDeviceCollector": "device_collector",
    "evaluation_collector": "device_collector",
    "GroupCollector": "group_collector",
    "BasicCollector": "basic_collector",
    "TrajectoryBuffer": "traj_buf",
})
