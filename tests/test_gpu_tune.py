"""rl_tune on the product library: "ablate" (kernel variants that are wrong by design) is a key of
the measurement build (-DRL_MEASURE=1) alone. The product refuses every value of it, 0 included,
and goes on deciding exactly as the oracle does."""
import numpy as np
import pytest

import rl_amd
from golden_io import load_traces
from oracle.coracle import COracle

pytestmark = pytest.mark.gpu


def test_ablate_is_no_key_of_the_product():
    d = load_traces()["mixed_small"]
    eng = rl_amd.Engine(device=0, max_batch=1 << 16, capacity=1 << 12)
    for l in d["limiters"]:
        eng.add_limiter(*l)
    for v in (0, 1, 256, 1 << 20):
        with pytest.raises(rl_amd.RlError) as err:
            eng.tune("ablate", v)
        assert err.value.status == rl_amd.RL_E_INVALID_ARG, v
    args = [d[k] for k in ("keys", "permits", "now_ns", "limiter", "op")]
    a, r, t, st = eng.execute(*args)
    oa, orem, ot, _ = COracle(d["limiters"]).run(*args)
    bad = np.nonzero((a != oa) | (r != orem))[0]
    assert bad.size == 0, f"{bad.size} decisions differ from the oracle (first {bad[:5]})"
    m = ~np.isnan(ot)
    assert np.array_equal(t[m].view(np.uint64), ot[m].view(np.uint64)), "token balances differ"
    assert st in (rl_amd.RL_OK, rl_amd.RL_E_INVALID_REQUEST), rl_amd.strerror(st)
