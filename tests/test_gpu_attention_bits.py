"""GPU: the flash self-attention kernels, the fused text + masked-IP cross-attention kernels (four-wave with and without T16,
the eight-wave ring, the long-prompt form) and the region-flags kernel give, bit for bit, what they gave before their row store,
softmax passes, Q load, panel staging and IP-side region logic were moved into shared device functions (csrc/ds_attention.h and
the shared section of csrc/attention.hip).  tests/_attention_bits_cases.py has the cases (integer-formula operands, no random
generator) and the recording; tests/golden/attention_bits.json holds the sha256 of every output as recorded on an MI355X from
the commit before that change.  The family's other tests compare the kernel variants with one another, or with fp64 references
at measured tolerances, which a reordered add inside a shared piece passes: the fixture is not to be re-recorded."""
import functools
import json

import pytest

from tests import _attention_bits_cases as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(C.FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_lists_exactly_the_cases():
    names = [C.case_name(group, case) for group, cases in C.GROUPS.items() for case in cases]
    assert len(names) == len(set(names)) and set(names) == set(_recorded())


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_attention_bits_are_the_recorded_ones(hip_lib, group):
    got = C.run_group(group)
    rec = _recorded()
    wrong = [name for name, digest in got.items() if rec[name] != digest]
    assert len(got) == len(C.GROUPS[group]) and not wrong, wrong
