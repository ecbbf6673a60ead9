"""The checkpoint file of packed state dicts (bzip3_amd.save_packed / load_packed / packed_index) and the metadata check of a chain of
them (bzip3_amd.check_chain), on the CPU: hand-made PackedTensors whose frames are CPU uint8 tensors.  No GPU and no library call.

The format, pinned here byte by byte ("Checkpoint files and batched checksums"): b"BZ3TNSR1", a little-endian u64 H, H bytes
of UTF-8 JSON padded with spaces so that 16 + H is a multiple of 64, then the frames in dict order, each at a multiple of 16 bytes from
the start of the data section."""
import json
import os
import shutil

import pytest
import torch

import bzip3_amd
from bzip3_amd import PackedTensor


def _frame(seed, n):
    return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _packed():
    """Five dtypes; shapes () and (0, 3) among them; a non-ASCII name; crc and base_crc both set and None."""
    return {
        "layer.0.weight": PackedTensor(_frame(1, 1000), torch.float32, torch.Size([10, 30]), 4, 65 * 1024, 1200, False, None, 0xDEADBEEF),
        "gewicht.ü.β": PackedTensor(_frame(2, 37), torch.bfloat16, torch.Size([7, 3]), 1, 70_000, 42, True, 0xFFFFFFFF, None),
        "flag": PackedTensor(_frame(3, 16), torch.bool, torch.Size([]), 1, 66_560, 1, False, None, None),
        "empty": PackedTensor(_frame(4, 13), torch.complex64, torch.Size([0, 3]), 4, 66_560, 0, True, 1, 1),
        "steps": PackedTensor(_frame(5, 4097), torch.int64, torch.Size([5]), 8, 1 << 20, 40, True, 0, 12345),
    }


FIELDS = ("dtype", "planes", "block_size", "nbytes", "delta", "base_crc", "crc")


def _same(p, q):
    return all(getattr(p, f) == getattr(q, f) for f in FIELDS) and tuple(p.shape) == tuple(q.shape) and torch.equal(p.frame.cpu(), q.frame.cpu())


@pytest.fixture()
def saved(tmp_path):
    path = str(tmp_path / "ckpt.bz3t")
    packed = _packed()
    meta = {"step": 7, "note": "größe", "nested": {"lr": 0.5, "tags": ["a", None, True]}}
    bzip3_amd.save_packed(path, packed, meta)
    return path, packed, meta


def _split(path):
    raw = open(path, "rb").read()
    hlen = int.from_bytes(raw[8:16], "little")
    return raw, hlen, json.loads(raw[16 : 16 + hlen].decode("utf-8"))


def _rewrite(path, out, edit=None, head_bytes=None, magic=b"BZ3TNSR1"):
    """A copy of the file with its JSON header edited (edit(header dict)) or replaced by head_bytes."""
    raw, hlen, head = _split(path)
    if head_bytes is None:
        edit(head)
        head_bytes = json.dumps(head, ensure_ascii=False).encode("utf-8")
    head_bytes += b" " * ((0 - (16 + len(head_bytes))) % 64)
    with open(out, "wb") as f:
        f.write(magic + len(head_bytes).to_bytes(8, "little") + head_bytes + raw[16 + hlen :])
    return out


def test_round_trip_every_field(saved):
    path, packed, meta = saved
    back = bzip3_amd.load_packed(path, "cpu")
    assert list(back) == list(packed)
    for k in packed:
        assert isinstance(back[k], PackedTensor) and _same(back[k], packed[k]), k
        assert back[k].frame.dtype == torch.uint8 and back[k].frame.device.type == "cpu"
        assert isinstance(back[k].dtype, torch.dtype) and isinstance(back[k].shape, torch.Size)
    assert back["gewicht.ü.β"].crc is None and back["flag"].base_crc is None and back["flag"].crc is None
    entries, got_meta = bzip3_amd.packed_index(path)
    assert got_meta == meta and list(entries) == list(packed)
    # an empty dict and no metadata
    bzip3_amd.save_packed(path, {})
    assert bzip3_amd.load_packed(path, "cpu") == {} and bzip3_amd.packed_index(path) == ({}, {})


def test_layout_is_pinned(saved):
    path, packed, meta = saved
    raw, hlen, head = _split(path)
    assert raw[:8] == b"BZ3TNSR1"
    assert (16 + hlen) % 64 == 0 and 16 + hlen <= len(raw)
    text = raw[16 : 16 + hlen]
    assert text.rstrip(b" ") == text.rstrip() and text.rstrip(b" ").endswith(b"}")  # padded with spaces alone
    assert "gewicht.ü.β".encode("utf-8") in text  # UTF-8, not \u escapes
    assert head["version"] == 1 and head["metadata"] == meta and list(head["tensors"]) == list(packed)
    end = 0
    for k, p in packed.items():
        e = head["tensors"][k]
        assert set(e) == {"dtype", "shape", "planes", "block_size", "nbytes", "delta", "base_crc", "crc", "offset", "size"}
        assert e["dtype"] == str(p.dtype).replace("torch.", "") and e["shape"] == list(p.shape)
        assert (e["planes"], e["block_size"], e["nbytes"], e["delta"], e["base_crc"], e["crc"]) == (p.planes, p.block_size, p.nbytes, p.delta, p.base_crc, p.crc)
        assert e["offset"] % 16 == 0 and e["offset"] >= end and e["offset"] - end < 16 and e["size"] == p.frame.numel()
        at = 16 + hlen + e["offset"]
        assert raw[at : at + e["size"]] == bytes(p.frame.numpy()), k  # the frame can be cut out by hand
        assert raw[16 + hlen + end : at] == b"\0" * (e["offset"] - end)  # zero padding between
        end = e["offset"] + e["size"]
    assert len(raw) == 16 + hlen + end


def test_subset_load_reads_only_its_ranges(saved, tmp_path):
    path, packed, _ = saved
    raw, hlen, head = _split(path)
    names = list(packed)
    first, last = names[0], names[-1]
    cut = str(tmp_path / "cut.bz3t")
    with open(cut, "wb") as f:
        f.write(raw[: 16 + hlen + head["tensors"][first]["offset"] + head["tensors"][first]["size"]])
    got = bzip3_amd.load_packed(cut, "cpu", names=[first])
    assert list(got) == [first] and _same(got[first], packed[first])
    with pytest.raises(ValueError):
        bzip3_amd.load_packed(cut, "cpu", names=[last])
    with pytest.raises(ValueError):
        bzip3_amd.load_packed(cut, "cpu")
    # the order asked for is the order returned, and each frame starts at a multiple of 16 bytes of one buffer
    got = bzip3_amd.load_packed(path, "cpu", names=[last, names[1]])
    assert list(got) == [last, names[1]] and all(_same(got[k], packed[k]) for k in got)
    assert (got[names[1]].frame.data_ptr() - got[last].frame.data_ptr()) == (packed[last].frame.numel() + 15) // 16 * 16


def test_packed_index_reads_no_frame(saved, tmp_path):
    path, packed, meta = saved
    raw, hlen, head = _split(path)
    only_header = str(tmp_path / "header.bz3t")
    with open(only_header, "wb") as f:
        f.write(raw[: 16 + hlen])
    entries, got_meta = bzip3_amd.packed_index(only_header)
    assert entries == head["tensors"] and got_meta == meta


def _set(name, key, value):
    def edit(head):
        head["tensors"][name][key] = value

    return edit


@pytest.mark.parametrize(
    "case",
    ["magic", "version", "header_past_file", "json", "dtype", "planes", "nbytes", "frame_past_file"],
)
def test_malformed_files(saved, tmp_path, case):
    path, packed, _ = saved
    raw, hlen, head = _split(path)
    bad = str(tmp_path / "bad.bz3t")
    index_fails = True
    if case == "magic":
        _rewrite(path, bad, edit=lambda h: None, magic=b"BZ3TNSR2")
    elif case == "version":
        _rewrite(path, bad, edit=lambda h: h.update(version=2))
    elif case == "header_past_file":
        with open(bad, "wb") as f:
            f.write(raw[:8] + (len(raw) - 15).to_bytes(8, "little") + raw[16:])
    elif case == "json":
        _rewrite(path, bad, head_bytes=raw[16 : 16 + hlen].rstrip(b" ")[:-1])
    elif case == "dtype":
        _rewrite(path, bad, edit=_set("flag", "dtype", "float33"))
    elif case == "planes":
        _rewrite(path, bad, edit=_set("steps", "planes", 3))
    elif case == "nbytes":
        _rewrite(path, bad, edit=_set("layer.0.weight", "nbytes", 1201))
    else:
        _rewrite(path, bad, edit=_set("steps", "size", 4098))
        index_fails = False  # the header itself is well formed: only loading that frame fails
    with pytest.raises(ValueError):
        bzip3_amd.load_packed(bad, "cpu")
    if index_fails:
        with pytest.raises(ValueError):
            bzip3_amd.packed_index(bad)
    else:
        bzip3_amd.packed_index(bad)
        assert list(bzip3_amd.load_packed(bad, "cpu", names=["flag"])) == ["flag"]


def test_truncated_fixed_part_is_a_value_error(tmp_path):
    short = str(tmp_path / "short.bz3t")
    with open(short, "wb") as f:
        f.write(b"BZ3TNSR1\x40")
    with pytest.raises(ValueError):
        bzip3_amd.packed_index(short)


def test_unknown_name_is_a_key_error(saved):
    path, _, _ = saved
    with pytest.raises(KeyError):
        bzip3_amd.load_packed(path, "cpu", names=["flag", "no such tensor"])


def test_save_is_atomic(saved, tmp_path):
    path, packed, _ = saved
    assert not os.path.exists(path + ".tmp")
    keep = str(tmp_path / "keep.bz3t")
    shutil.copy(path, keep)
    with pytest.raises(TypeError):
        bzip3_amd.save_packed(path, {"flag": packed["flag"]}, metadata={"unserialisable": object()})
    assert not os.path.exists(path + ".tmp")
    assert open(path, "rb").read() == open(keep, "rb").read(), "a failing save changed the existing file"
    # a good save replaces it
    bzip3_amd.save_packed(path, {"flag": packed["flag"]})
    assert list(bzip3_amd.load_packed(path, "cpu")) == ["flag"] and not os.path.exists(path + ".tmp")


# ---- check_chain ----------------------------------------------------------------------------------------------------------------
def _t(crc, base_crc=None, delta=False, dtype=torch.float32, shape=(4, 4), nbytes=64):
    return PackedTensor(_frame(9, 8), dtype, torch.Size(shape), 1, 65 * 1024, nbytes, delta, base_crc, crc)


def _chain():
    return [
        {"w": _t(11), "b": _t(21), "gone": _t(31)},
        {"w": _t(12, 11, True), "b": _t(22, 21, True), "new": _t(41)},  # "gone" is dropped, "new" comes whole
        {"w": _t(13, 12, True), "b": _t(23), "new": _t(42, 41, True)},   # "b" is replaced whole
    ]


def test_check_chain_passes_a_good_chain():
    assert bzip3_amd.check_chain(_chain()) == []
    assert bzip3_amd.check_chain([]) == [] and bzip3_amd.check_chain(_chain()[:1]) == []


def test_check_chain_names_the_step_and_the_tensor():
    c = _chain()
    c[2]["w"].base_crc = 99
    with pytest.raises(ValueError, match=r"step 2.*'w'"):
        bzip3_amd.check_chain(c)
    c = _chain()
    c[1]["b"] = _t(22, 21, True, shape=(2, 8))
    with pytest.raises(ValueError, match=r"step 1.*'b'"):
        bzip3_amd.check_chain(c)
    c = _chain()
    c[1]["b"] = _t(22, 21, True, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"step 1.*'b'"):
        bzip3_amd.check_chain(c)
    c = _chain()
    c[0]["b"] = _t(21, 5, True)
    with pytest.raises(ValueError, match=r"step 0.*'b'"):
        bzip3_amd.check_chain(c)
    c = _chain()
    del c[1]["new"]
    with pytest.raises(ValueError, match=r"step 2.*'new'"):
        bzip3_amd.check_chain(c)
    # the first violation is the one reported
    c = _chain()
    c[1]["w"].base_crc = 98
    c[2]["w"].base_crc = 99
    with pytest.raises(ValueError, match=r"step 1.*'w'"):
        bzip3_amd.check_chain(c)


def test_check_chain_returns_the_links_it_could_not_check():
    c = _chain()
    c[0]["w"].crc = None       # the link 0 -> 1 of "w"
    c[2]["new"].base_crc = None  # the link 1 -> 2 of "new"
    assert bzip3_amd.check_chain(c) == [(0, "w"), (1, "new")]


def test_chain_survives_the_file(tmp_path):
    steps = []
    for t, step in enumerate(_chain()):
        path = str(tmp_path / f"step{t}.bz3t")
        bzip3_amd.save_packed(path, step)
        steps.append(bzip3_amd.load_packed(path, "cpu"))
    assert bzip3_amd.check_chain(steps) == []
    steps[1]["w"].base_crc = 7
    with pytest.raises(ValueError, match=r"step 1.*'w'"):
        bzip3_amd.check_chain(steps)
