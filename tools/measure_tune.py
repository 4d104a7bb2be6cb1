"""rl_tune for the measurement tools. "ablate" is a key of the measurement build only, so the tools
leave it alone until a variant asks for a non-zero value, and say how to get that build when the
loaded library refuses it."""
import sys

import rl_amd

_ablated = False    # some engine of this process got a non-zero "ablate": zeros are passed on too


def tune(eng, key, value):
    global _ablated
    if key == "ablate":
        if not value and not _ablated:
            return                 # 0 is what every library does without being told
        _ablated = True
    try:
        eng.tune(key, value)
    except rl_amd.RlError as e:
        if key != "ablate" or e.status != rl_amd.RL_E_INVALID_ARG:
            raise
        sys.exit(f'{rl_amd.LIB_PATH} has no "ablate": build the measurement library with '
                 f'tools/build_variant.sh measure "-DRL_MEASURE=1" and set RL_ENGINE_LIB='
                 f'distributed-rate-limiter_amd/variants/measure/librl_engine.so')
