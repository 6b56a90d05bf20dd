"""GPU suite (-m gpu): k_tx_em's two ways through a class -- a lane for a list of up to TX_LONG_LIST (32) members, the whole wave for a longer one, 64 members
at a time -- against the sequential twin, as words.  The classes are put into the table with dg_tx_add, so every list length on either side of the seams (32 / 33,
64 / 65, 128 / 129) is there whatever reads would give: D is the members' theta added in ascending order in both ways, so the words equal the twin's exactly."""
import random
import numpy as np
import pytest
import common
import txquant_inputs as txi
from dart_amd import host

pytestmark = pytest.mark.gpu
N_TX = 600
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 600]


def _classes():
    rng = random.Random(5)
    classes = {}
    for n in LENGTHS + LENGTHS[:-1]:                                   # every length twice, over different members (the list of all of them once)
        classes[tuple(sorted(rng.sample(range(N_TX), n)))] = rng.randrange(1, 1000)
    while len(classes) < 700:                                          # short lists around them: more than two workgroups of classes, the long ones wherever their hashes put them
        classes[tuple(sorted(rng.sample(range(N_TX), rng.randrange(1, 6))))] = rng.randrange(1, 1000)
    return classes


def test_long_and_short_lists_give_the_twins_words(workdir):
    c = common.build_case("se100", workdir)
    tr = [(0, 0, [(100 + 40 * t, 110 + 40 * t + 3 * (t % 9))]) for t in range(N_TX)]         # lengths 10 .. 34: under the mean, eff_t = L_t
    L = txi.lengths(tr)
    classes = _classes()
    assert {len(k) for k in classes} >= set(LENGTHS) and sum(len(k) > 32 for k in classes) == 2 * sum(n > 32 for n in LENGTHS) - 1
    n = sum(classes.values())
    words = [n, 0, 0, 0, n, 0, 0, 0]
    gpu = host.DartGPU(host.Index(c["prefix"]), host.default_params(paired=0, max_mismatch=5))
    try:
        gpu.tx_set_annotation(*txi.annot_arrays(tr))
        gpu.tx_add(*txi.table_csr(classes), np.array(words, np.uint64))
        off, ids, cnt, w8 = gpu.tx_classes()
        assert txi.table_dict(off, ids, cnt) == classes and [int(x) for x in w8] == words
        for rounds in (0, 1, 16, 48):
            got = [int(x) for x in gpu.tx_finish(200, rounds)]
            ref = txi.em(classes, words, L, 200, rounds)
            print("max_rounds", rounds, "rounds", got[N_TX + 8], "converged", got[N_TX + 9], "EM ms", gpu.tx_em_device_ms)
            assert got == ref, [(t, a, b) for t, (a, b) in enumerate(zip(got, ref)) if a != b][:5]
    finally:
        gpu.close()
