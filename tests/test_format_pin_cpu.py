"""CPU tests of the path stage's pin (tests/golden/format/README.md): the goldens that tests/golden/make_golden_format.py recorded
from ntJoin's own find_paths and format_path on the generated inputs of tests/_format_cases.py are read back against their
digests, the conditions that keep them from going hollow are recomputed, and oracle/paths_oracle.py (find_paths, format_path) and
Ntjoin.determine_orientation are held to them: paths as ordered vertex lists, every row, and the ValueError where it was raised."""
import pytest

from oracle import graph_oracle as go
from oracle import paths_oracle as po
from tests import _format_cases as fc

SMALL = [(family, name) for family in ("fuzz", "m_rule", "gaps") for name, _g, _a in fc.family_specs()[family]]


def _oracle_answer(case, tmp_path):
    "-> (paths as lists of hash strings, rows per path, or None where the oracle's assert on the overhangs fired)"
    tsvs = fc.write_tsvs(case, str(tmp_path))
    state = go.load_and_build(tsvs[:-1], case["weights"][:-1], tsvs[-1], case["weights"][-1])
    filt = dict(state)
    if not case["n"] <= min(state["weights"].values()):      # the graph the scaffolder holds is the globally filtered one
        filt["edges"] = [e for e in state["edges"] if not e[3] < case["n"]]
    prepared = po.prepare_format(filt, tsvs[-1])
    paths = [p for comp in po.find_paths(state, case["n"]) for p in comp]
    rows = []
    for path in paths:
        try:
            rows.append(po.format_path(filt, path, tsvs[-1], case["lengths"], case["k"], case["g"], case["G"], case["m"], prepared=prepared))
        except AssertionError:
            rows.append(None)
    return paths, rows


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_goldens_load_and_their_conditions_hold(family):
    """load_family() re-makes every input and checks its digest; the conditions are those the recorder asserted"""
    entries = fc.load_family(family)
    assert len(entries) == len(fc.family_specs()[family])
    found = fc.check_conditions(family, entries)
    if family == "fuzz":
        print("fuzz counts:", found)
    if family == "gaps":
        for name, entry in entries.items():
            assert entry["meta"]["tags"] == entry["case"]["tags"] and entry["meta"]["doc"] == entry["case"]["doc"], name


@pytest.mark.parametrize("family,name", SMALL)
def test_oracle_equals_the_reference(family, name, tmp_path):
    """find_paths of the oracle gives the recorded paths as ordered vertex lists (direction counts, their order among themselves
    does not), format_path the recorded rows of each, and its assert fires exactly where the reference raised"""
    entry = fc.load_family(family)[name]
    paths, rows = _oracle_answer(entry["case"], tmp_path)
    want = {path: nodes for path, nodes in zip(entry["paths"], entry["rows"])}
    got = {tuple(int(v) for v in path): nodes for path, nodes in zip(paths, rows)}
    assert len(got) == len(paths) and set(got) == set(want)
    for path, nodes in want.items():
        assert got[path] == nodes, (name, entry["paths"].index(path))
    assert [p for p, nodes in enumerate(entry["rows"]) if nodes is None] == ([entry["error"]["path"]] if "error" in entry else [])


def test_oracle_equals_the_reference_on_the_wide_case(tmp_path):
    entry = fc.load_family("wide")["wide"]
    case = entry["case"]
    paths, rows = fc.pack(case, *_oracle_answer(case, tmp_path))
    got = fc.summarise_wide(paths, rows)
    for key in ("n_paths", "counts", "paths_head", "rows_head", "paths_sha256", "rows_sha256"):
        assert got[key] == entry[key], key


@pytest.mark.parametrize("name", [name for name, _g, _a in fc.family_specs()["m_rule"]])
def test_determine_orientation_equals_the_reference(name):
    """Ntjoin.determine_orientation on the run's (n, inc, dec) gives the orientation the reference gave U"""
    from ntjoin_amd.ntjoin import Ntjoin
    entry = fc.load_family("m_rule")[name]
    n, inc, dec = entry["case"]["u_pairs"]
    assert Ntjoin.determine_orientation(n, inc, dec, entry["case"]["m"]) == fc.u_orientation(entry)
