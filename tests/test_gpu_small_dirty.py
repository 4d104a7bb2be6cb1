"""The small-batch path on dirty device memory: every allocation of the library filled with a
chosen byte before use (rl_debug_alloc_fill; 0x00, 0xA5, 0xFF as tests/test_gpu_dirty_memory.py),
and the sizes, one-region and interleaving drivers of tests/small_cases.py still bit-exact against
the twin and the oracle. The path's scratch (records, packed results, runs, the touched list, its
control block and counters) is cleared nowhere: DESIGN.md §7a says per buffer which phase of the
kernel writes each word before another reads it. The 0x00 run must equal the unfilled run word
for word."""
import pytest

import rl_amd
import small_cases as sc

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)
DRIVERS = {
    "sizes-host": lambda: sc.run_sizes(),
    "sizes-device": lambda: sc.run_sizes(device=True),
    "one-region-fixed": lambda: sc.run_one_region(fixed=True),
    "one-region-grows": lambda: sc.run_one_region(fixed=False),
    "interleaving": lambda: sc.run_interleaving(n_big=60_000, n_small=20),
}


@pytest.fixture(params=FILLS, ids=lambda b: f"fill{b:02x}")
def fill(request):
    try:
        rl_amd.debug_alloc_fill(request.param)
        yield request.param
    finally:
        rl_amd.debug_alloc_fill(None)


def flat(out):
    return [x for batch in out for x in batch[:3]]


@pytest.mark.parametrize("name", list(DRIVERS))
def test_driver(fill, name):
    got = flat(DRIVERS[name]())                   # (asserts every batch against the twin and the oracle)
    if fill == 0x00:
        rl_amd.debug_alloc_fill(None)             # the control equals the unfilled run word for word
        plain = flat(DRIVERS[name]())
        assert len(plain) == len(got)
        for i, (p, g) in enumerate(zip(plain, got)):
            assert sc.same(p, g), f"{name} output {i}"
