"""CPU: every size function the library exports has a case that runs its buffer between guard bytes, or a stated reason why not.

The size functions are the exports whose names end in `_workspace`, `_workspace_full` or `_saved_bytes`.  tests/_guard.py keeps COVERED (size function ->
"test module::case") and EXEMPT (size function -> reason); a new size function fails here until it is entered in one of them, and a case that is renamed
or removed fails here until the table follows."""
import importlib

importlib.import_module("nerf-navigation_amd")

import _guard  # noqa: E402

SUFFIXES = ("_workspace", "_workspace_full", "_saved_bytes")


def size_functions():
    import ngp_hip
    return [name for name in ngp_hip.EXPORTS if name.endswith(SUFFIXES)]


def test_the_exports_hold_the_size_functions_the_table_knows():
    names = size_functions()
    assert len(names) == len(set(names)) >= 27 and "ngp_filter_occ_workspace" in names and "ngp_nav_run_saved_bytes" in names


def test_every_size_function_is_covered_or_exempt():
    names = size_functions()
    missing = [n for n in names if n not in _guard.COVERED and n not in _guard.EXEMPT]
    assert not missing, f"no guard case and no stated exemption for {missing}: add a case to tests/test_gpu_workspace_guard.py and enter it in tests/_guard.py"
    both = [n for n in names if n in _guard.COVERED and n in _guard.EXEMPT]
    assert not both, f"{both} are listed as covered and as exempt"
    stale = [n for n in list(_guard.COVERED) + list(_guard.EXEMPT) if n not in names]
    assert not stale, f"{stale} are in the table but no longer exported"


def test_the_named_cases_exist():
    for name, where in _guard.COVERED.items():
        module, _, case = where.partition("::")
        assert module and case.startswith("test_"), (name, where)
        assert callable(getattr(importlib.import_module(module), case, None)), f"{name}: {where} does not exist"


def test_every_exemption_states_its_reason():
    for name, reason in _guard.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 8, name
