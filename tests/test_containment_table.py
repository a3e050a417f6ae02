"""The containment table (tests/containment.py) against the headers, without a GPU: every entry point any header of
_lib.HEADERS declares is in a case of the table or in its exemption list with one of the two acceptable reasons, and every
call of every case restates its prototype -- arity, pointer or scalar per argument, const pointers only ever read, element
sizes.  A new entry point without a row fails here."""
import os

import pytest

import abi_support as abi
import containment as C


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def declared(L):
    protos = {}
    for header, _, _ in L.HEADERS:
        protos.update(abi.prototypes(os.path.join(abi.INCLUDE, header)))
    assert set(protos) == set(L.ALL_SIGNATURES)
    return protos


@pytest.fixture(scope="module")
def built(L):
    """Every case of the table, built (descriptions only: no device memory)."""
    return [(case_id, build(L)) for case_id, build in C.all_cases()]


def test_every_entry_point_is_in_the_table_or_exempt(declared, built):
    covered = {call.entry for _, calls in built for call in calls}
    assert covered <= set(declared), covered - set(declared)
    assert not covered & set(C.EXEMPT), covered & set(C.EXEMPT)
    missing = set(declared) - covered - set(C.EXEMPT)
    assert not missing, f"entry points with neither a row in tests/containment.py nor an exemption: {sorted(missing)}"
    assert set(C.EXEMPT) <= set(declared), set(C.EXEMPT) - set(declared)


def test_exemptions_carry_one_of_the_two_reasons(declared):
    for name, reason in C.EXEMPT.items():
        if reason == C.NO_DEVICE_WRITES:
            # such an entry takes no stream: it cannot enqueue anything (and no mutable device pointer but a host `out` struct)
            assert "plnerf_stream_t" not in declared[name][1], name
        else:
            assert reason.startswith("sentinel test: tests/"), (name, reason)
            path, test = reason[len("sentinel test: "):].split(" ")[0].split("::")
            source = open(os.path.join(abi.ROOT, path)).read()
            assert f"def {test}(" in source and "sentinel-filled" in source and "around8 == 0xA5" in source, (name, path, test)


def test_every_call_restates_its_prototype(L, declared, built):
    assert len({case_id for case_id, _ in built}) == len(built), "case ids are unique"
    for case_id, calls in built:
        C.case_buffers(calls)      # (one Buf per name)
        for call in calls:
            ret, params = declared[call.entry]
            assert ret == "int" and params[-1] == "plnerf_stream_t", call.entry
            C.check_against_prototype(call, params, L.ALL_SIGNATURES[call.entry][1])


def test_guards_come_from_the_size_queries(L):
    """The tile guards are the layout constants seen through the size queries: 256 rows of saved state, 192 rows of
    backward workspace -- whole multiples of a row in every precision."""
    lib = L.lib()
    for precision in C.PRECISIONS.values():
        saved, bwd = C._tile_guards(L, precision)
        assert saved > 0 and saved % 256 == 0 and bwd > 0 and bwd % 192 == 0
        if precision:      # (16-bit modes: rows padded to the tile, so 1 row costs what 256 do)
            assert int(lib.plnerf_mlp_saved_bytes(1, precision)) - int(lib.plnerf_mlp_saved_bytes(0, precision)) == saved
        else:              # (fp32: exactly n_rows rows)
            assert int(lib.plnerf_mlp_saved_bytes(1, precision)) * 256 == saved
