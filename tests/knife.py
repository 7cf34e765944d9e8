"""Knife-edge allowances are earned, and say what they let through.  A parity test may leave a chain out of its comparison with the oracle
only where the ORACLE's own run of that chain has a decision (an accept test, a step-size search's threshold) within `band` of its boundary:
`excused` asserts that for every chain that parted ways and fails the test otherwise, naming the chain, where it sits in the launch and the
first difference -- a chain that differs with no such decision behind it was computed wrongly.  The distances come from tests/oracle_margins.py;
tests/test_knife_margins_cpu.py asserts that for the seeds and models of tests/parity_cases.py no chain has one inside the band at all.

Every use of an allowance is reported as a warning -- pytest lists warnings at the end of a run whatever its verbosity -- with the test, the
chains and what was compared (`used`; the callers whose boundary is not an oracle decision of a chain, such as a resampling threshold, call
it themselves)."""
import warnings

import numpy as np


class KnifeEdge(UserWarning):
    pass


def used(where, **what):
    """Report a use of a knife-edge allowance.  where: the comparison; what: chain / step indices, the distance to the boundary, ..."""
    warnings.warn(KnifeEdge(f"knife-edge allowance used in {where}: " + ", ".join(f"{k}={v}" for k, v in what.items())), stacklevel=2)


def excused(where, parted, margin, band, first_bad=None, chain0=0):
    """Assert that every chain of `parted` (bool [C]) has margin < band, report each through `used` and return the mask of excused chains.
    margin (float [C]): the oracle's smallest distance to a decision boundary in that chain, up to and including the chain's first differing
    step where the test knows it, else over the whole run.  first_bad: {chain: its first difference (step, site, device value, oracle value,
    ...)}.  chain0: the global id of chain 0 (the random streams are keyed by global ids)."""
    parted, margin = np.asarray(parted, dtype=bool), np.asarray(margin, dtype=np.float64)
    assert parted.shape == margin.shape and parted.ndim == 1, (parted.shape, margin.shape)
    first_bad = first_bad or {}
    chains = [int(c) for c in np.nonzero(parted)[0]]

    def describe(c):
        return (f"chain {c} (global id {chain0 + c}, lane {c % 64} of wave {c // 64}): the oracle's margin is {margin[c]:.3e}, "
                f"first difference {first_bad.get(c, 'not located')}")

    unexcused = [c for c in chains if not margin[c] < band]              # (a NaN margin excuses nothing)
    assert not unexcused, (f"{where}: {len(unexcused)} of {parted.size} chains differ from the oracle with no decision within {band:g} of its "
                           f"boundary -- not a knife edge, the device computed something else:\n  " + "\n  ".join(describe(c) for c in unexcused[:8]))
    for c in chains:
        used(where, chain=c, global_id=chain0 + c, lane=c % 64, wave=c // 64, margin=float(margin[c]), band=band, first_difference=first_bad.get(c))
    return parted.copy()
