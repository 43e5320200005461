"""Shared by the tests of the one-pass self-critical step (sc_samples >= 2) and by the script that writes their fixtures
(tests/golden/make_golden_sc_samples.py): loading, the rule by which a large gradient is stored as a sample of its entries, and the
brute-force "mean of the others" in exact rational arithmetic."""
import os
import zlib
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NS_CASE = (2, 3, 5)                                  # fixture (a): samples per caption row
NS_TRAIN = (2, 3)                                    # fixture (b)
MODELS = ("subgc_train", "fullgc_train")
FULL_BELOW, SAMPLE = 4096, 1024                      # a gradient of more than FULL_BELOW entries is stored as SAMPLE of them plus its norm
EPS = 2.0 ** -53


def load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def sample_index(name, numel):
    """The flat entries of parameter `name`'s gradient that fixture (b) stores: all of them up to FULL_BELOW entries, else SAMPLE distinct
    ones drawn from a generator seeded by the name (ascending).  A committed file is limited to 1 MiB; four cases of every gradient in
    full are five times that."""
    if numel <= FULL_BELOW:
        return None
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return np.sort(rng.choice(numel, SAMPLE, replace=False))


def stored_gradient(name, g):
    """-> {key: array} of one gradient as the fixture stores it."""
    g = np.asarray(g)
    idx = sample_index(name, g.size)
    if idx is None:
        return {name: g}
    return {name + "#sample": g.reshape(-1)[idx], name + "#norm": np.float64(np.linalg.norm(g.astype(np.float64)))}


def loo_fraction(scores, n):
    """Brute force in exact arithmetic: reward of row k b5 + s = s_k - mean of the OTHER samples' scores of caption row s.
    -> (reward, baseline) as lists of Fraction, sample-major like the input."""
    s = [Fraction(float(x)) for x in np.asarray(scores, np.float64).reshape(-1)]
    b5 = len(s) // n
    reward, baseline = [None] * len(s), [None] * len(s)
    for c in range(b5):
        for k in range(n):
            others = [s[j * b5 + c] for j in range(n) if j != k]
            baseline[k * b5 + c] = sum(others) / (n - 1)
            reward[k * b5 + c] = s[k * b5 + c] - baseline[k * b5 + c]
    return reward, baseline
