"""The JavaScript host's SimCluster.leave / rejoin / flags (tests/js/
test_lifecycle.js) on the 10-node case of the reference-recorded fixture
tests/golden/sim_lifecycle.json.gz."""
import os
import subprocess

import pytest

from test_js import NODE, ROOT, build_addon

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_lifecycle():
    build_addon()
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_lifecycle.js")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "js lifecycle ok" in r.stdout
