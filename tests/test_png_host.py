"""png.py and the evaluation's image writers, without a GPU: write_png / read_png round-trip the three array kinds the
package writes (byte order of 16-bit samples and odd sizes included), the files are well-formed PNG (signature, chunk
CRCs, filter type 0) and decode to the same pixels in PIL where PIL is installed; write_images_with_metrics and
write_images_with_metrics_testdist name their directory as run_plnerf.py:365-415 does and write to8b / to16b of the
frames they are given."""
import binascii
import contextlib
import io
import os
import struct
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from plnerf_amd import evaluate as E
from plnerf_amd import png

RNG = np.random.default_rng(7)


def _images():
    order = np.zeros((3, 5), dtype=np.uint16)
    order[0, 0], order[0, 1], order[2, 4], order[1, 2] = 0x00FF, 0xFF00, 0x1234, 0xFFFF
    return {
        "rgb_5x3": RNG.integers(0, 256, (5, 3, 3), dtype=np.uint8),
        "rgb_1x1": np.array([[[1, 2, 3]]], dtype=np.uint8),
        "rgb_16x24": RNG.integers(0, 256, (16, 24, 3), dtype=np.uint8),
        "grey8_5x3": RNG.integers(0, 256, (5, 3), dtype=np.uint8),
        "grey16_5x3": RNG.integers(0, 65536, (5, 3), dtype=np.uint16),
        "grey16_byte_order": order,
        "grey16_1x7": RNG.integers(0, 65536, (1, 7), dtype=np.uint16),
    }


@pytest.mark.parametrize("name", sorted(_images()))
def test_round_trip_and_file_structure(tmp_path, name):
    a = _images()[name]
    path = tmp_path / (name + ".png")
    png.write_png(str(path), a)
    back = png.read_png(str(path))
    assert back.dtype == a.dtype and back.shape == a.shape and np.array_equal(back, a)
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    # the chunks, walked independently of png.chunks: lengths add up to the file, every CRC verifies
    at, kinds, idat = 8, [], b""
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == binascii.crc32(kind + payload) & 0xffffffff, kind
        kinds.append(kind)
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", payload)
        if kind == b"IDAT":
            idat += payload
        at += 12 + n
    assert at == len(data) and kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and b"IDAT" in kinds
    H, W = a.shape[:2]
    depth, colour = (16 if a.dtype == np.uint16 else 8), (2 if a.ndim == 3 else 0)
    assert header == (W, H, depth, colour, 0, 0, 0)
    raw = zlib.decompress(idat)
    stride = W * (3 if a.ndim == 3 else 1) * (depth // 8)
    assert len(raw) == H * (1 + stride)
    assert all(raw[r * (1 + stride)] == 0 for r in range(H))                         # filter type 0 on every row
    if a.dtype == np.uint16:                                                          # big-endian samples
        first = raw[1:1 + stride]
        assert [first[2 * k] * 256 + first[2 * k + 1] for k in range(W)] == a[0].tolist()
    assert png.chunks(data) and [k for k, _ in png.chunks(data)] == kinds


def test_byte_order_of_16_bit_samples_in_the_file(tmp_path):
    a = _images()["grey16_byte_order"]
    raw = zlib.decompress(b"".join(p for k, p in png.chunks(png.encode_png(a)) if k == b"IDAT"))
    assert raw[1:5] == b"\x00\xff\xff\x00"


@pytest.mark.parametrize("name", sorted(_images()))
def test_pil_decodes_the_same_pixels(tmp_path, name):
    Image = pytest.importorskip("PIL.Image")
    a = _images()[name]
    path = tmp_path / (name + ".png")
    png.write_png(str(path), a)
    with Image.open(str(path)) as im:
        got = np.asarray(im)
    assert got.shape == a.shape and np.array_equal(got.astype(np.int64), a.astype(np.int64))


def test_write_png_refuses_other_arrays_and_read_png_damaged_files(tmp_path):
    for bad in (np.zeros((4, 4), dtype=np.float32), np.zeros((4, 4, 4), dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.uint16),
                np.zeros((0, 4), dtype=np.uint8), np.zeros(4, dtype=np.uint8)):
        with pytest.raises(ValueError):
            png.write_png(str(tmp_path / "bad.png"), bad)
    data = bytearray(png.encode_png(_images()["rgb_5x3"]))
    data[45] ^= 1                                                                     # inside IDAT: its CRC no longer verifies
    (tmp_path / "damaged.png").write_bytes(bytes(data))
    with pytest.raises(ValueError):
        png.read_png(str(tmp_path / "damaged.png"))
    (tmp_path / "not.png").write_bytes(b"GIF89a" + bytes(20))
    with pytest.raises(ValueError):
        png.read_png(str(tmp_path / "not.png"))


def test_trailing_axis_of_one_is_a_grey_image(tmp_path):
    a = RNG.integers(0, 65536, (4, 5, 1), dtype=np.uint16)
    png.write_png(str(tmp_path / "d.png"), a)
    assert np.array_equal(png.read_png(str(tmp_path / "d.png")), a[:, :, 0])


# ----------------------------------------------------------------------------- the evaluation's writers
def _res(n=2, H=5, W=4):
    g = torch.Generator().manual_seed(3)
    res = {"rgbs": torch.rand(n, 3, H, W, generator=g), "target_rgbs": torch.rand(n, 3, H, W, generator=g),
           "depths": torch.rand(n, 1, H, W, generator=g)}
    # code boundaries, and values a clamp has to catch (the writers clip as to8b / to16b do)
    res["rgbs"][0, :, 0, 0] = torch.tensor([0.0, 1.0, 254.0 / 255.0])
    res["rgbs"][1, :, 0, 1] = torch.tensor([1.5, -0.25, 0.5])
    res["depths"][0, 0, 0, :3] = torch.tensor([0.0, 1.0, 255.0 / 65535.0])
    res["depths"][1, 0, 1, 0] = 1.25
    return res


def _tracker():
    m = E.MeanTracker()
    m.add({"img_loss": 0.0123, "psnr": 19.1, "ssim": 0.61})
    m.add({"img_loss": 0.0100, "psnr": 20.0, "ssim": 0.65, "depth_rmse": 0.3})
    return m


def _to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def _to16b(x):
    return (65535 * np.clip(x, 0, 1)).astype(np.uint16)


def _check_dir(result_dir, res, tracker, printed):
    assert sorted(os.listdir(result_dir)) == sorted([f"{n}_{k}.png" for n in range(2) for k in ("rgb", "gt", "d")] + ["metrics.txt"])
    for n in range(2):
        rgb = res["rgbs"][n].permute(1, 2, 0).numpy()
        gt = res["target_rgbs"][n].permute(1, 2, 0).numpy()
        d = res["depths"][n].permute(1, 2, 0).numpy()
        assert np.array_equal(png.read_png(os.path.join(result_dir, f"{n}_rgb.png")), _to8b(rgb))        # RGB order
        assert np.array_equal(png.read_png(os.path.join(result_dir, f"{n}_gt.png")), _to8b(gt))
        got_d = png.read_png(os.path.join(result_dir, f"{n}_d.png"))
        assert got_d.dtype == np.uint16 and np.array_equal(got_d, _to16b(d)[:, :, 0])
    want = io.StringIO()
    tracker.print(want)
    assert open(os.path.join(result_dir, "metrics.txt")).read() == want.getvalue() == printed
    assert "psnr: " in want.getvalue() and "depth_rmse: " in want.getvalue()


@pytest.mark.parametrize("opt,samples,name", [
    (False, False, "test_images_linear_64_128scene0710_00"),
    (True, False, "test_images_linear_64_128with_optimization_scene0710_00"),
    (False, True, "test_images_sampleslinear_64_12864_128scene0710_00"),
    (True, True, "test_images_sampleslinear_64_128with_optimization_64_128scene0710_00"),
])
def test_write_images_with_metrics(tmp_path, opt, samples, name):
    args = Namespace(ckpt_dir=str(tmp_path), expname="exp", mode="linear", N_samples=64, N_importance=128, scene_id="scene0710_00")
    res, tracker = _res(), _tracker()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        E.write_images_with_metrics(res, tracker, 6.0, args, with_test_time_optimization=opt, test_samples=samples)
    assert os.listdir(os.path.join(str(tmp_path), "exp")) == [name]
    _check_dir(os.path.join(str(tmp_path), "exp", name), res, tracker, out.getvalue())


@pytest.mark.parametrize("opt,samples,dist,name", [
    (False, False, 0.25, "test_images_dist0.25_scene0710_00"),
    (True, False, 1, "test_images_dist1_with_optimization_scene0710_00"),
    (False, True, 0.5, "test_images_samples_dist0.5_64_128scene0710_00"),
    (True, True, 2.0, "test_images_samples_dist2.0_with_optimization_64_128scene0710_00"),
])
def test_write_images_with_metrics_testdist(tmp_path, opt, samples, dist, name):
    args = Namespace(ckpt_dir=str(tmp_path), expname="exp", mode="constant", N_samples=64, N_importance=128, scene_id="scene0710_00")
    res, tracker = _res(), _tracker()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        E.write_images_with_metrics_testdist(res, tracker, 6.0, args, dist, with_test_time_optimization=opt, test_samples=samples)
    assert os.listdir(os.path.join(str(tmp_path), "exp")) == [name]
    _check_dir(os.path.join(str(tmp_path), "exp", name), res, tracker, out.getvalue())
