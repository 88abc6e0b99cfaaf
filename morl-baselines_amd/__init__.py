"""morl-baselines_amd: MI355X-native (gfx950) hot path of the morl-baselines TD update.

Host code is Python on PyTorch-ROCm and mirrors the reference's class API (MOPolicy / MOAgent /
ReplayBuffer / pareto helpers); the arithmetic runs in hand-written HIP kernels behind the C ABI of
``include/morl_hip.h`` (``lib/libmorl_hip.so``).  There is no CPU fallback.
"""
__version__ = "0.1.0"

from . import native, ops  # noqa: F401
from .native import load_library  # noqa: F401


def __getattr__(name):
    # the agents import torch.nn modules and, where present, the reference's base classes: loaded on first use
    if name == "PCN":
        from .pcn import PCN
        return PCN
    if name == "LCN":
        from .lcn import LCN
        return LCN
    if name in ("MOPPO", "MOPPONet"):
        from . import mo_ppo
        return getattr(mo_ppo, name)
    if name in ("NLMOPPO", "Agent"):
        from . import nl_mo_ppo
        return getattr(nl_mo_ppo, name)
    if name == "EUPG":
        from .eupg import EUPG
        return EUPG
    if name in ("IPRO", "OuterLoop"):
        from . import ipro
        return getattr(ipro, name)
    if name == "PGMORL":
        from .pgmorl import PGMORL
        return PGMORL
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
