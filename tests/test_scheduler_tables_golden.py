"""Every table the device sees from a scheduler, and every construction outcome, against the dump of the commit before
the four schedulers were put on one base class (tests/golden/scheduler_tables.npz, written by
tools/dump_scheduler_tables.py).  CPU only, no library, no tolerance: a bit moved in a table, a dtype, a refusal or a
`.config` fails."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_scheduler_tables",
                                               os.path.join(ROOT, "tools", "dump_scheduler_tables.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "scheduler_tables.npz")) as npz:
        return dump.unpack(npz)


@pytest.fixture(scope="module")
def current():
    """The matrix from the working tree, generated with the shared library out of reach: the tables are host arithmetic
    (`ops` binds the library at the first launch, not on import)."""
    from diffsensei_amd import _lib

    def no_library():
        raise AssertionError("a scheduler table loaded the HIP library")

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "load", no_library)
        return dump.collect()


def test_the_matrix_is_whole(golden):
    arrays, outcomes = golden
    # 2 (Euler, DDIM) + 3 spacings x 2 karras x 2 final x 2 solver_type x 2 solver_order x 2 lower_order_final
    # + 1 euler_at_final (DPM) + 3 spacings (Euler a), each at 6 step counts
    entries = {key.rsplit("/", 1)[0] for key in arrays}
    assert len(dump.table_matrix()) == 2 + 96 + 1 + 3 and len(dump.STEPS) == 6
    assert len(entries) == 102 * 6
    fields = {"euler": 4, "ddim": 3, "dpm": 6, "euler_a": 4}     # timesteps, init_noise_sigma, coef_table [, sigmas
    assert len(arrays) == 6 * (4 + 3 + 97 * 6 + 3 * 4)           # [, solver_table, step_orders]]
    for name, count in fields.items():
        lead = name if name in ("euler", "ddim") else f"{name}/leading" + ("/karras0/zero/midpoint/order2/lof1" * (name == "dpm"))
        for n in dump.STEPS:
            assert sum(key.startswith(f"{lead}/n{n}/") for key in arrays) == count, (lead, n)
    # 19 + 7 refusals of the DPM / Euler a tests and 10 x 2 of the Euler / DDIM loop, through both routes; 5 x 4 swaps
    assert len(outcomes) == 2 * (19 + 7 + 10 * 2) + 5 * 4
    refused = [key for key, o in outcomes.items() if "raises" in o]
    assert all(outcomes[key] == {"raises": "NotImplementedError"} for key in refused)
    # every listed key refused by its constructor; `from_config` drops the 3 + 5 keys Euler / DDIM do not list, and of
    # the swaps only Euler refuses (a Karras DPM config)
    assert sum(" constructor " in key for key in refused) == 19 + 7 + 10 * 2
    assert sum(" from_config " in key and " of " not in key for key in refused) == 19 + 7 + 10 * 2 - 3 - 5
    assert [key for key in refused if " of " in key] == \
        ["EulerDiscreteScheduler from_config of DPMSolverMultistepScheduler(karras)"]
    assert len(refused) == 85


def test_the_tool_lists_the_refusals_of_the_scheduler_tests():
    from tests.test_dpm_scheduler import REFUSED as dpm_refused
    from tests.test_euler_ancestral_scheduler import REFUSED as euler_a_refused
    assert dump.DPM_REFUSED == dpm_refused and dump.EULER_A_REFUSED == euler_a_refused


def test_tables_are_bit_identical(golden, current):
    want, got = golden[0], current[0]
    assert sorted(got) == sorted(want)
    bad = [key for key, a in want.items()
           if not (got[key].dtype == a.dtype and got[key].shape == a.shape and np.array_equal(got[key], a, equal_nan=True))]
    assert not bad, (len(bad), bad[:10])


def test_construction_outcomes_are_identical(golden, current):
    want, got = golden[1], current[1]
    assert sorted(got) == sorted(want)
    bad = {key: (got[key], o) for key, o in want.items() if got[key] != o}
    assert not bad, bad
