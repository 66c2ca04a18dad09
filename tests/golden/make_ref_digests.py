"""Writes tests/golden/ref_digests.npz: per test that holds code against the reference's own (oracle/_ref/libref_probe.so), one
64-bit digest per iteration of its loop over what the REFERENCE returned (orc.RefAnswers).  Where oracle/_ref cannot be built
those tests hold the oracle and the host library to these digests instead of skipping.  Run where oracle/_ref is built:
    make -C oracle && python tests/golden/make_ref_digests.py
Fixtures are data (digests of outputs); no reference source text is stored."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TESTS = {"oracle_vs_reference_live": "tests/test_oracle_pins.py::test_oracle_vs_reference_live",
         "oracle_bvh_vs_reference_live": "tests/test_oracle_pins.py::test_oracle_bvh_vs_reference_live",
         "oracle_vs_reference_live_on_special_values": "tests/test_oracle_pins.py::test_oracle_vs_reference_live_on_special_values",
         "oracle_bvh_vs_reference_live_on_awkward_meshes": "tests/test_oracle_pins.py::test_oracle_bvh_vs_reference_live_on_awkward_meshes",
         "host_math_vs_reference_instance_build": "tests/test_host_logic.py::test_host_math_on_special_values_vs_oracle"}

if __name__ == "__main__":
    assert os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_probe.so")), "oracle/_ref missing: run `make -C oracle` where the reference is mounted"
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, RT_RECORD_REF_DIGESTS=d)
        subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + list(TESTS.values()), cwd=ROOT, env=env, check=True)
        out = {k: np.load(os.path.join(d, k + ".npy")) for k in TESTS}
    np.savez_compressed(os.path.join(HERE, "ref_digests.npz"), **out)
    print({k: v.shape[0] for k, v in out.items()})
