"""CPU suite: the synthetic genome's i.i.d. codes drawn in parallel chunks (dart_amd/synth.py::_uniform_codes) are numpy's single
rng.integers(0, 4, uint8) call, and leave the generator where that call leaves it."""
import numpy as np
import pytest
from dart_amd import synth


@pytest.mark.parametrize("seed,total", [(20, 1 << 24), (91, 8 * 3_000_017), (5, 8 * 2_500_001 + 4), (3, 4096)])
def test_uniform_codes_are_the_single_call(seed, total):
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    assert np.array_equal(synth._uniform_codes(a, total), b.integers(0, 4, size=total, dtype=np.uint8))
    # what make_genome draws next: scalars, uint8 and double arrays
    assert int(a.integers(0, 3_000_000_000)) == int(b.integers(0, 3_000_000_000))
    assert np.array_equal(a.integers(1, 4, size=1001, dtype=np.uint8), b.integers(1, 4, size=1001, dtype=np.uint8))
    assert np.array_equal(a.random(999), b.random(999))
