"""north_star: "keeping the src/models nn.Module API surface so the existing train.py/evaluate.py drive it unchanged".

The ``src`` shim (``src/__init__.py``) gives the model the reference's module path (``src.models.cabinet``) without
shadowing the reference's own ``src`` package: with ``PYTHONPATH=<repo>:<reference checkout>`` (INTEGRATION.md path A) the
modules this repository provides resolve here and every other ``src.*`` module resolves to the checkout behind it.  The
checkout is stood in for by a tree generated under ``tmp_path`` with the package layout the reference's scripts import from
(regular packages, the namespace directory ``src/scripts``, the subpackage ``src/models/layers``), so the test needs nothing
outside this repository."""
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]

# what this repository provides: the model and the loss (the generated tree holds a decoy of each, which must not win)
MINE = ("src.models.cabinet", "src.models.cab", "src.models.constants", "src.models.mobilenetv3", "src.utils.loss")
# what the reference's train.py / evaluate.py import besides them (train.py:18-31): found behind this repository
THEIRS = ("src.utils.optimizer", "src.utils.ema", "src.utils.early_stopping", "src.utils.exceptions", "src.utils.logger",
          "src.utils.class_weights", "src.datasets.registry", "src.scripts.evaluate", "src.scripts.train", "src.models.layers")


def _stand_in_checkout(root):
    """src/, src/models/, src/utils/, src/datasets/ and src/models/layers/ as regular packages, src/scripts/ without an
    __init__.py; the two scripts import the model and the loss by the reference's module path, as the real ones do."""
    for pkg in ("src", "src/models", "src/utils", "src/datasets", "src/models/layers"):
        (root / pkg).mkdir(parents=True, exist_ok=True)
        (root / pkg / "__init__.py").write_text("")
    (root / "src" / "scripts").mkdir()
    for mod in MINE + THEIRS:
        path = root / (mod.replace(".", "/") + ".py")
        if not path.parent.joinpath(path.stem, "__init__.py").exists():
            path.write_text("")
    uses = "from src.models.cabinet import CABiNet  # noqa: F401\nfrom src.utils.loss import OhemCELoss  # noqa: F401\n"
    for script in ("train", "evaluate"):
        (root / "src" / "scripts" / f"{script}.py").write_text(uses)


def test_shim_does_not_shadow_the_reference_package(tmp_path):
    """Every module reference train.py:18-31 imports resolves: the model + loss to this repo, the rest to the reference."""
    ref = tmp_path / "reference"
    _stand_in_checkout(ref)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(REPO), str(ref)]), PYTHONDONTWRITEBYTECODE="1")
    code = (
        "import json, src, src.models.cabinet, src.models.cab, src.models.constants, src.models.mobilenetv3, src.utils.loss\n"
        "import src.utils.optimizer, src.utils.ema, src.utils.early_stopping, src.utils.exceptions, src.utils.logger\n"
        "import src.utils.class_weights, src.datasets.registry, src.scripts.evaluate, src.scripts.train, src.models.layers\n"
        "import sys\n"
        "print(json.dumps({m: sys.modules[m].__file__ for m in sorted(sys.modules) if m.startswith('src.') and "
        "getattr(sys.modules[m], '__file__', None)}))\n")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    files = json.loads(out.stdout.strip().splitlines()[-1])
    mine = set(MINE) | {"src.models", "src.utils"}
    for mod, f in files.items():
        root = REPO if mod in mine else ref
        assert Path(f).is_relative_to(root), f"{mod} resolved to {f}, expected under {root}"
    for mod in ("src.utils.optimizer", "src.utils.ema", "src.scripts.train", "src.scripts.evaluate", "src.datasets.registry",
                "src.models.layers"):
        assert mod in files
