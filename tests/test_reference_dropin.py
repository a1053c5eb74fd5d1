"""CPU: ``optimizer`` / ``loss`` / ``train`` under the reference's import names drive the device layers after
``np_modeling_amd.install()`` (BASELINE.json north_star: "Trainer/optimizer/loss drop in unchanged"; reference
train.py:20-46, optimizer.py:13-18,53-67, loss.py:21-39, train_test.py:14-81).

The modules are the reference's own, unchanged, when NPM_REFERENCE names a checkout of it, and this package's versions
of the same contract otherwise; the expected values are recorded fixtures either way.  The flows run in a child
interpreter (tests/dropin_worker.py) so that the top-level module names are bound only there."""

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_modules_drive_installed_layers():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    env.pop('PYTHONPATH', None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'dropin_worker.py')], env=env,
                          capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert 'DROPIN OK' in proc.stdout
    assert 'train_mlp[sgd]' in proc.stdout and 'train_mlp[adam]' in proc.stdout
