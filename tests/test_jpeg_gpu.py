"""decode_jpeg_batch / GPUJpegDecoder / image_loader on the device, on top of the kernels that tests/test_jpeg_kernels_gpu.py
checks through the C-ABI.  The reference is the fixture's PIL arrays (tests/golden/jpeg_cases.npz); everything is integers, so
the bound is equality.  PIL is not needed here."""
import math

import pytest
import torch

import jpeg_util as JU
from vision_toolbox import _native as N
from vision_toolbox import data as D

pytestmark = pytest.mark.gpu

CASES = JU.cases()


def same_batch(batch, ref):
    assert batch.raw.device.type == "cuda" and batch.table.device.type == "cuda" and batch.status.device.type == "cuda"
    assert batch.raw.dtype == torch.uint8 and batch.table.dtype == torch.int64 and batch.status.dtype == torch.int32
    assert torch.equal(batch.raw.cpu(), ref.raw), int((batch.raw.cpu() != ref.raw).sum())
    assert torch.equal(batch.table.cpu(), ref.table) and batch.sizes == ref.sizes


def test_decode_jpeg_batch_is_from_images_of_the_pil_arrays():
    mixed = JU.mixed()
    before = N.launch_count()
    batch = D.decode_jpeg_batch([c.data for c in mixed], "cuda")
    torch.cuda.synchronize()
    assert N.launch_count() == before + 2  # the two launches, nothing else from the library
    same_batch(batch, D.RaggedBatch.from_images([c.rgb for c in mixed]))
    assert batch.status.tolist() == [0] * len(mixed)
    # the CPU path is the host stage: the same batch
    cpu = D.decode_jpeg_batch([c.data for c in mixed], "cpu")
    assert torch.equal(cpu.raw, batch.raw.cpu()) and torch.equal(cpu.table, batch.table.cpu()) and cpu.status.tolist() == batch.status.tolist()


def test_decoder_object_keeps_its_scratch_and_takes_a_band_height():
    dec = D.GPUJpegDecoder(band_mcu_rows=1)
    everything = list(CASES.values())
    big = dec([c.data for c in everything], "cuda")
    same_batch(big, D.RaggedBatch.from_images([c.rgb for c in everything]))
    assert len(dec._scratch) == 1
    scratch = next(iter(dec._scratch.values()))
    staged = {k: v.data_ptr() for k, v in dec._staging[str(big.raw.device)].items()}
    assert set(staged) >= {"data", "images", "segments", "qtabs", "hufftabs", "table"} and all(v.is_pinned() for v in dec._staging[str(big.raw.device)].values())
    small = dec([c.data for c in JU.mixed()], "cuda")
    same_batch(small, D.RaggedBatch.from_images([c.rgb for c in JU.mixed()]))
    assert next(iter(dec._scratch.values())) is scratch and len(dec._scratch) == 1  # a smaller batch reuses it
    assert {k: v.data_ptr() for k, v in dec._staging[str(big.raw.device)].items()} == staged  # and the pinned staging buffers
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # another stream gets a scratch of its own
        other = dec([c.data for c in JU.mixed()], "cuda")
    side.synchronize()
    assert len(dec._scratch) == 2 and torch.equal(other.raw, small.raw)
    assert big.status.tolist() == [0] * len(everything)


def test_status_names_the_damaged_image():
    c = CASES["420_53x37_noise_q90_r3"]
    cut = c.data[: (c.info.scan_offset + c.info.scan_end) // 2]
    files = [CASES["gray_17x9_noise_q90"].data, cut, CASES["444_8x8_noise_q90"].data]
    batch = D.decode_jpeg_batch(files, "cuda")
    host = D.decode_jpeg_batch(files, "cpu")
    assert batch.status.tolist() == host.status.tolist() == [0, D.JPEG_ERR_TRUNCATED, 0]
    assert torch.equal(batch.raw.cpu(), host.raw)  # zeros from the failing block on: both sides decode them to the same levels


def test_image_loader(tmp_path):
    c = CASES["420_53x37_noise_q75_r2_spliced"]
    p = tmp_path / "a.jpg"
    p.write_bytes(c.data)
    got = D.image_loader(str(p), "cuda")
    assert got.device.type == "cuda" and got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(got.cpu(), c.rgb.permute(2, 0, 1))
    assert torch.equal(D.image_loader(p), c.rgb.permute(2, 0, 1))


def test_decoded_batch_feeds_the_train_step():
    """batch = decode_jpeg_batch(files, "cuda"); aug(batch, params, out=ts.images); ts.step() -- the same bits in ts.images as
    feeding the PIL-decoded batch, and the step runs on them"""
    from oracle import filler
    from vision_toolbox import backbones
    from vision_toolbox.trainer import TrainStep

    picked = [CASES[n] for n in ("420_53x37_noise_q90", "422_53x37_gradient_q90", "444_53x37_noise_q75", "420_40x48_noise_q90")]
    B, S, ncls = len(picked), 32, 8
    ts = TrainStep(backbones.darknet_yolov5n(), ncls, B, S, torch.float32, lr=0.01, device="cuda", deterministic=True)
    filler.fill_module(ts.model, "jpeg.")
    ts.weights_changed()
    aug = D.GPUBatchTransform(S)
    batch = D.decode_jpeg_batch([c.data for c in picked], "cuda")
    params = D.sample_train_params(batch.sizes, S, erase_p=0.5, generator=torch.Generator().manual_seed(11))
    assert aug(batch, params, out=ts.images).data_ptr() == ts.images.data_ptr()
    fed = ts.images.clone()
    ref = D.RaggedBatch.from_images([c.rgb for c in picked]).to("cuda")
    assert torch.equal(aug(ref, params), fed)
    assert torch.equal(aug(batch, params, out=ts.images), fed)
    ts.step(labels=filler.labels(B, ncls).cuda())
    assert math.isfinite(ts.loss()) and torch.equal(ts.images, fed)
