"""GPU tests of the path stage against ntJoin's own answers on generated inputs (tests/golden/format/README.md): per case of the
four families of tests/_format_cases.py, MxEngine.find_paths must give exactly the recorded paths (as vertex-hash lists, direction
included) and mxg_format_paths (MxEngine.format_paths, Ntjoin.format_paths) exactly the recorded rows of each, all nine columns;
where the reference raised ValueError the library's error names that path and node and every other path still has its rows."""
import re

import pytest

from tests import _format_cases as fc
from tests.test_gpu_format_paths import _Host, _add, _check_segments, _rows

pytestmark = pytest.mark.gpu


def _names(family):
    return [name for name, _g, _a in fc.family_specs()[family]]


def _library_answer(entry):
    """-> (paths as tuples of vertex hashes, rows per path), after the checks every case gets: the segments, Ntjoin.format_paths
    through _Host, and where the golden holds an error, the error"""
    from ntjoin_amd.engine import MxEngine, MxError
    case = entry["case"]
    order = fc.asm_names(case)
    tgt = len(order) - 1
    kw = dict(g=case["g"], G=case["G"], m=case["m"])
    with MxEngine(k=32, w=10) as eng:
        for name, weight, records in zip(order, case["weights"], case["asms"]):
            _add(eng, name, weight, records)
        eng.build_graph()
        found = eng.find_paths(case["n"])
        vh = eng.get_graph()["vertex_hash"]
        paths = [tuple(vh[verts].tolist()) for _comp, verts in found]
        ids = eng.record_ids(tgt, eng.n_records(tgt))
        host = _Host(eng, order, found)
        if "error" not in entry:
            nodes = eng.format_paths(tgt, lengths=[case["lengths"][c] for c in ids], **kw)
            rows = _rows(eng, tgt, nodes)
            assert host.nj.format_paths(case["lengths"], kw["g"], kw["G"], kw["m"], False) == rows
        else:
            err = entry["error"]
            with pytest.raises(MxError) as ei:
                eng.format_paths(tgt, lengths=[case["lengths"][c] for c in ids], **kw)
            nodes = ei.value.nodes
            assert nodes is not None and "less than 0" in str(ei.value)
            rows = _rows(eng, tgt, nodes)
            where = re.search(r"path (\d+) node (\d+)", str(ei.value))
            p, j = int(where.group(1)), int(where.group(2))
            assert paths[p] == entry["paths"][err["path"]] and (rows[p][j][0], rows[p][j + 1][0]) == (err["u"], err["v"])
            with pytest.raises(ValueError) as ev:
                host.nj.format_paths(case["lengths"], kw["g"], kw["G"], kw["m"], False)
            assert f"less than 0 between ['{err['u']}'" in str(ev.value) and f" and ['{err['v']}'" in str(ev.value)
            rows[p] = None
        assert len(nodes["node_first"]) == len(found) + 1
        _check_segments(eng, tgt, nodes)
    return paths, rows


def _check_case(entry):
    paths, rows = _library_answer(entry)
    want = dict(zip(entry["paths"], entry["rows"]))
    got = dict(zip(paths, rows))
    assert len(got) == len(paths) and set(got) == set(want)
    for path, nodes in want.items():
        assert got[path] == nodes, entry["paths"].index(path)


@pytest.mark.parametrize("name", _names("fuzz"))
def test_fuzz_equals_the_reference(name):
    """60 draws of the generator of test_fuzz_against_host_route (its 12 trials are the first 12), m in {50, 75, 90}, g in {1, 20},
    G in {0, 40}, n in {1, 2}"""
    _check_case(fc.load_family("fuzz")[name])


@pytest.mark.parametrize("name", _names("m_rule"))
def test_m_rule_equals_the_reference(name):
    """one path A - U - C: U's orientation where inc / float(d) * 100 >= m and exact arithmetic part, at exact boundaries, m = 100,
    m = 50 with half the pairs, two minimizers"""
    entry = fc.load_family("m_rule")[name]
    _check_case(entry)


@pytest.mark.parametrize("name", _names("gaps"))
def test_gaps_equal_the_reference(name):
    """hand-made junctions: orientation pairs, whole and cut contigs, 1 to 3 supporting assemblies and the truncation of their mean,
    raw around g and G, stretches of 1 to 300 edges, empty support, paths of unoriented runs, the two negative overhangs"""
    _check_case(fc.load_family("gaps")[name])


def test_wide_equals_the_reference():
    """1500 paths in one call: the scans and node_first run over several blocks, the junction waves over many"""
    entry = fc.load_family("wide")["wide"]
    paths, rows = _library_answer(entry)
    packed = fc.pack(entry["case"], [[str(h) for h in path] for path in paths], rows)
    got = fc.summarise_wide(*packed)
    for key in ("n_paths", "counts", "paths_head", "rows_head", "paths_sha256", "rows_sha256"):
        assert got[key] == entry[key], key
