"""librvb_test.so is "the same objects plus test_api.hip" (README.md, csrc/common.h, csrc/test_api.h):
reverb_amd/build.py links every object into both libraries but one a side, the two definitions of lab_env()."""
import os

from reverb_amd import build


def stems(sources):
    return {os.path.splitext(s)[0] for s in sources}


def test_the_two_libraries_differ_by_lab_env_off_and_test_api():
    assert set(build.LINK) == {build.OUT, build.OUT_TEST}
    product, lab = build.LINK[build.OUT], build.LINK[build.OUT_TEST]
    for s in product + lab:                 # plain file names: no source is built a second time under another stem or with other flags
        assert isinstance(s, str) and os.path.isfile(os.path.join(build.CSRC, s)), s
    assert len(stems(product)) == len(product) and len(stems(lab)) == len(lab)
    assert stems(product) - stems(lab) == {"lab_env_off"}
    assert stems(lab) - stems(product) == {"test_api"}
    assert {"engine", "engine_weights", "engine_encode", "engine_decode", "engine_ctc"} <= stems(product) & stems(lab)
