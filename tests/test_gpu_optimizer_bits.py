"""GPU: the optimiser's bytes are those of the commit tests/golden/optimizer_bits.json names -- every rule on both access paths,
plain and clipped, trainable and frozen; the trust passes; the norm and the clip block.  The cases and how the fixture was
written: tests/optimizer_bits.py.  The other optimiser tests hold the kernels to a bar against numpy; this one fixes every
rounding, RMSProp's split between its 16-byte path (a fused multiply-add for the mean square) and its element path (a product
and a sum) among them.  Every digest is equal; none is ever regenerated from the code under test.
"""
import json

import pytest

from tests import optimizer_bits as OB
from tests.test_gpu_optimizer import gpu  # noqa: F401  (the fixture)

GROUPS = OB.groups()


def golden():
    with open(OB.GOLDEN) as f:
        return json.load(f)


def test_fixture_names_exactly_the_cases():
    gold = golden()
    assert sorted(gold["digests"]) == sorted(k for ks in GROUPS.values() for k in ks)
    assert len(gold["parent"]) == 40 and all(len(d) == 64 for d in gold["digests"].values())


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_bytes_are_the_recorded_ones(gpu, group):  # noqa: F811
    torch, l = gpu
    want = golden()["digests"]
    got = {key: OB.run(torch, l, key) for key in GROUPS[group]}
    differ = [key for key in GROUPS[group] if got[key] != want[key]]
    assert not differ, "bytes changed: %s" % differ
