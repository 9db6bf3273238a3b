"""``include/fedagg.h``, the table of ``tests/stream_contract_cases.py`` and the cases of
``tests/test_stream_contract_gpu.py``, kept in step: an entry point that takes a ``void* stream``
and has neither side-stream / graph-replay cases nor a stated reason turns this red."""

import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg.h"


def stream_prototypes(header: Path):
    """Names of the prototypes whose last parameter is ``void* stream`` (comments stripped; the
    ``#if FEDAGG_TUNING`` block counts: the table says why its entry is left out)."""
    text = re.sub(r"/\*.*?\*/", " ", header.read_text(), flags=re.S)
    names = []
    for m in re.finditer(r"\b(fedagg_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        if re.fullmatch(r"void\s*\*\s*stream", params[-1]):
            names.append(m.group(1))
    return names


def problems(header: Path, table, case_entries):
    """Every disagreement between the header, the table and the GPU file's cases."""
    out = []
    protos = stream_prototypes(header)
    if len(set(protos)) != len(protos):
        out.append("a prototype is declared twice")
    out += [f"{n}: takes a stream but has no table entry" for n in protos if n not in table]
    out += [f"{n}: in the table but not a prototype with a trailing `void* stream`" for n in table if n not in protos]
    claimed = set()
    for name, e in table.items():
        if set(e) == {"excluded"}:
            if not (isinstance(e["excluded"], str) and e["excluded"].strip()):
                out.append(f"{name}: excluded without a reason")
        elif set(e) == {"cases"}:
            if not e["cases"]:
                out.append(f"{name}: neither cases nor a reason")
            for cid in e["cases"]:
                if cid not in case_entries:
                    out.append(f"{name}: no case {cid} in tests/test_stream_contract_gpu.py")
                elif name not in case_entries[cid]:
                    out.append(f"{name}: case {cid} does not call it (it calls {case_entries[cid]})")
                claimed.add(cid)
        else:
            out.append(f"{name}: an entry is either cases or excluded")
    out += [f"case {cid}: no table entry lists it" for cid in case_entries if cid not in claimed]
    for cid, entries in case_entries.items():
        out += [f"case {cid} calls {n}, whose table entry does not list it" for n in entries
                if cid not in table.get(n, {}).get("cases", [])]
    return out


def _loaded():
    import test_stream_contract_gpu as gpu_test
    from stream_contract_cases import TABLE

    assert len(set(gpu_test.CASE_IDS)) == len(gpu_test.CASE_IDS)
    return TABLE, gpu_test.CASE_ENTRIES


def test_header_parse_finds_the_stream_entry_points():
    protos = stream_prototypes(HEADER)
    assert len(protos) == 49 and len(set(protos)) == 49, len(protos)
    assert {"fedagg_fedavg_f32", "fedagg_push_execute", "fedagg_copy_async", "fedagg_flat_increment_kind",
            "fedagg_read_probe_tile_f32"} <= set(protos)
    assert "fedagg_session_stage" not in protos and "fedagg_tune" not in protos


def test_table_header_and_cases_agree():
    table, case_entries = _loaded()
    assert problems(HEADER, table, case_entries) == []


def test_a_missing_entry_or_a_new_prototype_is_noticed(tmp_path):
    """The check itself: it turns red for a dropped entry, a new prototype, an empty entry and an
    unknown case id."""
    table, case_entries = _loaded()
    dropped = {k: v for k, v in table.items() if k != "fedagg_cast"}
    assert any("fedagg_cast: takes a stream" in p for p in problems(HEADER, dropped, case_entries))
    grown = tmp_path / "fedagg.h"
    grown.write_text(HEADER.read_text().replace("#ifdef __cplusplus\n}", "int fedagg_new_thing(const float* d_x, "
                                                "uint64_t n,\n                     void* stream);\n#ifdef __cplusplus\n}"))
    assert "fedagg_new_thing" in stream_prototypes(grown)
    assert any("fedagg_new_thing: takes a stream" in p for p in problems(grown, table, case_entries))
    assert any("neither cases nor a reason" in p for p in problems(HEADER, {**table, "fedagg_cast": {"cases": []}},
                                                                   case_entries))
    assert any("excluded without a reason" in p for p in problems(HEADER, {**table, "fedagg_cast": {"excluded": " "}},
                                                                  case_entries))
    assert any("no case cast-u8-f64" in p for p in problems(HEADER, {**table, "fedagg_cast": {"cases": ["cast-u8-f64"]}},
                                                            case_entries))


def test_header_lists_the_exclusions():
    """The header names, next to its "capturable" sentence, the entry points the promises do not cover."""
    table, _ = _loaded()
    opening = HEADER.read_text().split("#ifndef FEDAGG_H")[0]
    for name, e in table.items():
        assert (name in opening) == ("excluded" in e), name
