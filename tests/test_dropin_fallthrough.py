"""The drop-in boundary on its own (no reference tree needed; tests/test_dropin_imports.py replays the reference drivers' imports
where that tree is present): with ``dropin/`` first on sys.path, the shimmed modules hand out the MI355X implementation's hot-path
names, and any other name falls through to the module of the same name further down sys.path (dropin/_delegate.py), loaded under
a private alias -- here a stand-in written to tmp_path, whose own imports of shimmed modules resolve through the drop-in as well."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shims_serve_the_package_and_fall_through_to_the_next_module(tmp_path):
    shadow = tmp_path / "shadow"
    (shadow / "metrics").mkdir(parents=True)
    (shadow / "metrics" / "__init__.py").write_text("def scalar_metric(a, b):\n    return 'shadowed metrics'\n")
    (shadow / "evaluate.py").write_text(textwrap.dedent('''
        from metrics import scalar_metric, dice_coef        # resolved through the drop-in, like any driver's import
        def evaluate_scalar():
            return scalar_metric(0, 0)
        def uses_device_dice():
            return dice_coef.__module__
    '''))
    prog = textwrap.dedent('''
        import sys
        sys.path.insert(0, %r)          # the stand-in (shadowed)
        sys.path.insert(0, %r)          # the drop-in, first
        import model, train, inference, evaluate, metrics
        assert type(model.nets).__module__.startswith("cellsegmentation_amd") or model.nets.__name__.startswith("cellsegmentation_amd")
        assert train.train_tile.__module__.startswith("cellsegmentation_amd")
        assert inference.inference_tiles.__module__.startswith("cellsegmentation_amd")
        assert inference.sample.__module__.startswith("cellsegmentation_amd")
        assert evaluate.evaluate_tile.__module__.startswith("cellsegmentation_amd")
        assert metrics.dice_coef.__module__.startswith("cellsegmentation_amd")
        # names the package does not provide come from the next module of that name, under a private alias
        assert evaluate.evaluate_scalar.__module__ == "_shadowed_evaluate"
        assert evaluate.evaluate_scalar() == "shadowed metrics"
        assert evaluate.uses_device_dice().startswith("cellsegmentation_amd")
        assert metrics.scalar_metric.__module__ == "_shadowed_metrics"
        try:
            metrics.no_such_name
        except AttributeError:
            pass
        else:
            raise AssertionError("an unknown name must raise AttributeError")
        print("OK")
    ''') % (str(shadow), os.path.join(ROOT, "dropin"))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:]
