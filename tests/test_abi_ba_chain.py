"""The chained GN loop's test and tool entry points (include/vo_hip_testing_chain.h): declared in
a header of their own, exported by the library and bound in _lib.py; none of them in the product
header or in vo_hip_testing.h (no GPU)."""

import re

from visualodometry_amd import _lib


def _functions(path):
    text = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", text)))


def test_chain_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    names = _functions(_lib.CHAIN_TEST_HEADER)
    assert names == ["vo_ba_testing_chain_poll", "vo_ba_testing_chain_stamps", "vo_ba_testing_last_run",
                     "vo_ba_testing_no_chain"]
    assert sorted(_lib.CHAIN_SIGNATURES) == names
    for n in names:
        fn = getattr(lib, n)
        assert fn.argtypes == _lib.CHAIN_SIGNATURES[n][1], n
    other = set(_functions(_lib.HEADER)) | set(_functions(_lib.TEST_HEADER))
    assert not other & set(names)


def test_chain_switches_validate_arguments():
    lib = _lib.load()
    assert lib.vo_ba_testing_no_chain(None, 1) == _lib.VO_ERR_ARG
    assert lib.vo_ba_testing_chain_poll(None, 1) == _lib.VO_ERR_ARG
    assert lib.vo_ba_testing_last_run(None, None, None) == _lib.VO_ERR_ARG
