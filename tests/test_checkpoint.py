"""Checkpoint interop: the YOLOv5 key grammar of scripts/convert_yolov5_weights.py:6-52,
extras.extract_backbone_weights (extras.py:112-128), and save -> reference format -> load round trips.

What the unmodified reference makes of the files this package writes (its converter's output keys, its backbones'
state_dict and feature maps after loading them) is recorded by tools/gen_golden_checkpoint.py in
tests/golden/checkpoint_*.npz."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import filler
from vision_toolbox import backbones, checkpoint


@pytest.fixture(scope="module")
def manifest(golden_dir):
    return json.loads((golden_dir / "manifest.json").read_text())


def _gold(golden_dir, stem):
    with np.load(golden_dir / f"checkpoint_{stem}.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("variant", ["n", "x"])
def test_yolov5_key_grammar(variant, manifest, tmp_path, golden_dir):
    keys = [k for k, _ in manifest[f"darknet_yolov5{variant}"]["keys"]]
    mapped = [checkpoint.toolbox_to_yolov5_key(k) for k in keys]
    assert len(set(mapped)) == len(keys)
    assert [checkpoint.yolov5_to_toolbox_key(k) for k in mapped] == keys
    # the documented rules (convert_yolov5_weights.py:10-16)
    rules = {"stem.conv.weight": "model.0.conv.weight", "stages.0.conv.norm.bias": "model.1.norm.bias",
             "stages.0.conv1.conv.weight": "model.2.cv2.conv.weight", "stages.0.conv2.conv.weight": "model.2.cv1.conv.weight",
             "stages.1.blocks.1.conv2.norm.weight": "model.4.m.1.cv2.norm.weight",
             "stages.3.out_conv.conv.weight": "model.8.cv3.conv.weight"}
    for k, v in rules.items():
        assert checkpoint.toolbox_to_yolov5_key(k) == v and checkpoint.yolov5_to_toolbox_key(v) == k
    with pytest.raises(ValueError, match="Unexpected weight name"):
        checkpoint.toolbox_to_yolov5_key("head.weight")
    # the unmodified script must produce the same file: its keys, in its order, and every tensor passed through as is
    m = getattr(backbones, f"darknet_yolov5{variant}")()
    src, b = tmp_path / "src.pth", tmp_path / "b.pth"
    checkpoint.save_backbone(m, src)
    checkpoint.convert_yolov5_weights(src, b, verbose=False)
    ss, sb = torch.load(src), torch.load(b)
    assert list(sb) == [str(k) for k in _gold(golden_dir, "convert")[f"convert/{variant}/keys"]]
    assert len(sb) == len(ss) and all(torch.equal(sb[k], ss[k0]) for k, k0 in zip(sb, ss))
    checkpoint.convert_yolov5_weights(b, tmp_path / "c.pth", to="toolbox", verbose=False)
    sc = torch.load(tmp_path / "c.pth")
    assert list(sc) == list(ss) and all(torch.equal(sc[k], ss[k]) for k in ss)


def test_extract_backbone_weights(tmp_path):
    bb = backbones.vovnet19_slim_ese()
    model = torch.nn.Sequential(bb, torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(512, 10))
    filler.fill_module(model, "ckpt.")
    lightning = {"state_dict": {"model." + k: v for k, v in model.state_dict().items()}, "epoch": 3}
    torch.save(lightning, tmp_path / "last.ckpt")
    path = checkpoint.extract_backbone_weights(tmp_path / "last.ckpt", "vovnet19_slim_ese", tmp_path)
    data = Path(path).read_bytes()
    assert Path(path).name == f"vovnet19_slim_ese-{hashlib.sha256(data).hexdigest()[:8]}.pth"
    sd = torch.load(path)
    assert list(sd) == list(bb.state_dict()) and not any(k.startswith(("1.", "3.")) for k in sd)
    fresh = backbones.vovnet19_slim_ese()
    fresh.load_state_dict(sd)
    x = filler.images(1, 64)
    bb.eval(), fresh.eval()
    with torch.no_grad():
        torch.testing.assert_close(fresh(x), bb(x))


@pytest.mark.parametrize("name", ["cspdarknet53", "darknet_yolov5n", "vovnet19_slim_ese"])
def test_saved_checkpoint_loads_into_the_unmodified_reference(name, tmp_path, golden_dir, manifest):
    gold = _gold(golden_dir, name)
    ours = getattr(backbones, name)()
    filler.fill_module(ours, "rt.")
    ours._vt_runner().store.ensure(torch.device("cpu"))  # flat channels_last storage, as after a GPU run
    path = tmp_path / f"{name}.pth"
    checkpoint.save_backbone(ours, path)
    sd = torch.load(path)
    assert all(v.is_contiguous() for v in sd.values())
    # what the reference's strict load_state_dict() checks: same keys, same OIHW shapes as its own state_dict
    ref_keys = [str(k) for k in gold[f"rt/{name}/keys"]]
    assert sorted(sd) == sorted(ref_keys)
    assert {k: list(sh) for k, sh in manifest[name]["keys"]} == {k: list(v.shape) for k, v in sd.items()}
    x = filler.images(2, 64)
    ours.eval()
    with torch.no_grad():
        a = ours.get_feature_maps(x)
    b = [torch.from_numpy(gold[f"rt/{name}/map{i}"]) for i in range(len(a))]  # the reference on the loaded file
    assert f"rt/{name}/map{len(a)}" not in gold
    for u, v in zip(a, b):
        assert u.shape == v.shape
        assert ((u - v).norm() / v.norm()).item() < 1e-5  # (channels_last filter strides pick another ATen kernel)
    # and back: a file written by the reference (its state_dict: its key order and dtypes, the values it loaded) loads here
    dtypes = dict(zip(ref_keys, (str(d) for d in gold[f"rt/{name}/dtypes"])))
    torch.save({k: sd[k].to(getattr(torch, dtypes[k].split(".")[-1])) for k in ref_keys}, tmp_path / "ref.pth")
    again = getattr(backbones, name)()
    again.load_state_dict(torch.load(tmp_path / "ref.pth"))
    with torch.no_grad():
        assert ((again.eval()(x) - b[-1]).norm() / b[-1].norm()).item() < 1e-5


@pytest.mark.gpu
def test_gpu_module_round_trips_through_the_reference_format(tmp_path):
    """train one step on the GPU (weights, running statistics and counters change inside the flat store),
    save in the reference's format, load into a fresh module and into the CPU oracle"""
    from oracle import torch_ref as R

    m = backbones.darknet_yolov5n()
    filler.fill_module(m, "rt.")
    m = m.cuda().train()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    x = filler.images(4, 64).cuda()
    m(x).square().mean().backward()
    opt.step()
    path = tmp_path / "y5n.pth"
    checkpoint.save_backbone(m, path)
    sd = torch.load(path)
    assert all(v.device.type == "cpu" and v.is_contiguous() for v in sd.values())
    assert int(sd["stem.norm.num_batches_tracked"]) == 1
    m.eval()
    with torch.no_grad():
        got = m.get_feature_maps(x)
        ref = R.feature_maps("darknet_yolov5n", {k: v.clone() for k, v in sd.items()}, x.cpu(), False)
    for a, b in zip(got, ref):
        assert ((a.float().cpu() - b).norm() / b.norm()).item() < 1e-3
    fresh = backbones.darknet_yolov5n()
    fresh.load_state_dict(sd)
    with torch.no_grad():
        torch.testing.assert_close(fresh.cuda().eval()(x), got[-1], rtol=1e-4, atol=1e-4)
