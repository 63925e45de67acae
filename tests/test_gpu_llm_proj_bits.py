"""GPU: the four LLM projection kernels of csrc/llm.hip give, bit for bit, what they gave before their row staging, weight
load and output element were moved into shared device functions.  tests/_llm_proj_cases.py has the cases (integer-formula
operands, no random generator, no quantiser) and the recording; tests/golden/llm_proj_bits.json holds the sha256 of every
output as recorded on an MI355X from the commit before that change.  A case that differs is a changed summation order or
rounding point in the kernel, which the tolerance tests of these kernels would pass: the fixture is not to be re-recorded."""
import functools
import json

import pytest

from tests import _llm_proj_cases as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(C.FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_lists_exactly_the_cases():
    names = [C.case_name(*key, e, M) for key, cases in C.GROUPS.items() for e, M in cases]
    assert len(names) == len(set(names)) and set(names) == set(_recorded())


@pytest.mark.parametrize("kernel,fmt,shape", list(C.GROUPS), ids=["-".join(k) for k in C.GROUPS])
def test_projection_bits_are_the_recorded_ones(hip_lib, kernel, fmt, shape):
    got = C.run_group(kernel, fmt, shape)
    rec = _recorded()
    wrong = [name for name, digest in got.items() if rec[name] != digest]
    assert len(got) == len(C.GROUPS[kernel, fmt, shape]) and not wrong, wrong
