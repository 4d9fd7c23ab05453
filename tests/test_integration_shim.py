"""CPU: the reference-side shim integration/i3d_mi355x.py exercised the way the reference's plugin loader
(altfreezing/utils/plugin_loader.py:27-52) and ModelBase lifecycle (model/_base.py:39-104) use it:
get_classifier("i3d_mi355x")() -> .eval() -> .load(wrapped checkpoint) -> state_dict keys == the reference layout.
The host tree is a stand-in built in a temporary directory from the contract recorded in tests/golden/plugin_host.json
(oracle/gen_golden.py --plugin-host): a ``config`` singleton with the yaml's clip geometry, the plugin package, and a
loader that imports ``<package>.<name>`` and takes its ``Classifier``.  Runs in a child process: the stand-in's
top-level packages (config, model) go into sys.modules."""
import json
import os
import subprocess
import sys

from conftest import ROOT, load_json

SCRIPT = r'''
import importlib, json, os, sys, tempfile
ROOT, HOST = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, HOST)
import torch
host = json.load(open(os.path.join(ROOT, "tests", "golden", "plugin_host.json")))


def get_classifier(name):                                    # the loader's contract: <package>.<name> -> its Classifier
    return getattr(importlib.import_module(host["package"] + "." + name.replace("-", "_")), host["attribute"])


plugins = importlib.import_module(host["package"])          # the host's plugin package
plugins.__path__.append(os.path.join(ROOT, "integration"))  # = "copy i3d_mi355x.py next to i3d_ori.py"
os.environ["AF_MI355X_ROOT"] = ROOT
Cls = get_classifier("i3d_mi355x")                           # what `classifier_type: i3d_mi355x` resolves to
clf = Cls()
clf.eval()
from af_mi355x import synth
sd = synth.synthetic_state_dict(seed=0)
with tempfile.TemporaryDirectory() as td:
    p = os.path.join(td, "w.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, p)
    ok = clf.load(p)
    missing = clf.load(os.path.join(td, "nope.pth"))
got = clf.network.state_dict()
try:
    clf(torch.zeros(1, 3, 32, 224, 224))
    cpu_call = "ran"
except RuntimeError as e:
    cpu_call = "RuntimeError: " + str(e)[:60]
print(json.dumps({
    "class": Cls.__name__, "module": Cls.__module__, "clip": clf.network.clip_size,
    "load": list(ok), "load_missing": list(missing),
    "layout": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in got.items()],
    "loaded_equal": all(torch.equal(got[k], sd[k]) for k in sd),
    "has_surface": all(hasattr(clf, a) for a in ("network", "_warped_network", "load", "forward", "module_to_build")),
    "host_surface": sorted(a for a in host["surface"] if hasattr(Cls, a)),
    "cpu_call": cpu_call,
}))
'''


def _host_tree(root, host):
    """A minimal host tree: config.config carries the yaml's clip_size / imsize; <package> is an empty package."""
    with open(os.path.join(root, "config.py"), "w") as f:
        f.write("class _Config:\n    clip_size = %d\n    imsize = %d\n\n\nconfig = _Config()\n" % (host["clip_size"], host["imsize"]))
    d = root
    for part in host["package"].split("."):
        d = os.path.join(d, part)
        os.makedirs(d)
        open(os.path.join(d, "__init__.py"), "w").close()


def test_shim_through_the_reference_plugin_loader(tmp_path):
    host = load_json("plugin_host.json")
    _host_tree(str(tmp_path), host)
    r = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["class"] == "Classifier" and out["module"] == "model.classifier.i3d_mi355x"
    assert out["clip"] == 32                                        # read from the host's config singleton
    assert out["load"] == [True, -1] and out["load_missing"] == [False, -1]
    lay = load_json("layout.json")
    assert out["layout"] == lay["entries"] and len(out["layout"]) == 320
    assert out["loaded_equal"] and out["has_surface"]
    assert out["host_surface"] == host["surface"] == ["forward", "freeze", "load", "module_to_build"]
    assert out["cpu_call"].startswith("RuntimeError")              # no CPU fallback behind the plugin surface either
