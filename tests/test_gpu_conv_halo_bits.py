"""GPU: the three halo-patch convolution kernels of csrc/conv_halo.hip give, bit for bit, what they gave before their tile
decode, patch / weight descriptors, fragment walk and epilogue were moved into shared device functions.
tests/_conv_halo_cases.py has the cases (integer-formula operands, no random generator) and the recording;
tests/golden/conv_halo_bits.json holds the sha256 of every output as recorded on an MI355X from the commit before that change.
The family's other tests compare the three kernels with one another (torch.equal across conv_halo_variant 1 / 2 / 3), which a
change that moves all three together - a reordered add in the shared epilogue, say - passes: the fixture is not to be re-recorded."""
import functools
import json

import pytest

from tests import _conv_halo_cases as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(C.FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_lists_exactly_the_cases():
    names = [C.case_name(*key, *case) for key, cases in C.GROUPS.items() for case in cases]
    assert len(names) == len(set(names)) and set(names) == set(_recorded())


@pytest.mark.parametrize("kernel,inst", list(C.GROUPS), ids=["-".join(k) for k in C.GROUPS])
def test_conv_halo_bits_are_the_recorded_ones(hip_lib, kernel, inst):
    got = C.run_group(kernel, inst)
    rec = _recorded()
    wrong = [name for name, digest in got.items() if rec[name] != digest]
    assert len(got) == len(C.GROUPS[kernel, inst]) and not wrong, wrong
