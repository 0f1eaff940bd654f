"""Helpers for the -m gpu parity tests: pitched device surfaces backed by torch uint8 tensors.

torch is used only as a device allocator / copy engine here; every conversion goes through the C ABI.
"""
from __future__ import annotations

import numpy as np
import torch

PAD = 0xCD


def round_up(v, a):
    return (v + a - 1) // a * a


class DevPlanes:
    """Device copy of a list of numpy planes, each in its own pitched allocation.

    pitch = round_up(row_bytes, align) + extra; padding bytes are 0xCD and can be verified untouched.
    `offset` shifts the first byte of every plane (to exercise unaligned base pointers).
    All planes get the SAME (align, extra, offset): LaidOutPlanes takes one per plane, or stacks the planes in one allocation.
    """

    def __init__(self, host_planes, align=256, extra=0, offset=0, device="cuda:0"):
        self.host_shapes = [(p.shape, p.dtype) for p in host_planes]
        self.bufs, self.pitches, self.offset = [], [], offset
        for p in host_planes:
            rows, rb = p.shape[0], p.shape[1] * p.dtype.itemsize
            pitch = round_up(rb, align) + extra
            h = np.full((rows * pitch + offset + 64,), PAD, dtype=np.uint8)
            view = h[offset:offset + rows * pitch].reshape(rows, pitch)
            view[:, :rb] = p.view(np.uint8).reshape(rows, rb)
            self.bufs.append(torch.from_numpy(h).to(device))
            self.pitches.append(pitch)

    def desc(self):
        return [(b.data_ptr() + self.offset, pitch) for b, pitch in zip(self.bufs, self.pitches)]

    def upload(self, host_planes):
        """new pixels into the SAME device buffers (a captured graph keeps their addresses)"""
        for b, pitch, p in zip(self.bufs, self.pitches, host_planes):
            rows, rb = p.shape[0], p.shape[1] * p.dtype.itemsize
            h = np.full((rows * pitch + self.offset + 64,), PAD, dtype=np.uint8)
            h[self.offset:self.offset + rows * pitch].reshape(rows, pitch)[:, :rb] = p.view(np.uint8).reshape(rows, rb)
            b.copy_(torch.from_numpy(h))

    def download(self):
        """-> (list of tight numpy planes, padding_intact: bool)"""
        out, intact = [], True
        for b, pitch, (shape, dt) in zip(self.bufs, self.pitches, self.host_shapes):
            rows, rb = shape[0], shape[1] * np.dtype(dt).itemsize
            h = b.cpu().numpy()
            body = h[self.offset:self.offset + rows * pitch].reshape(rows, pitch)
            out.append(np.ascontiguousarray(body[:, :rb]).view(dt).reshape(shape))
            intact &= bool((body[:, rb:] == PAD).all()) and bool((h[:self.offset] == PAD).all()) and bool(
                (h[self.offset + rows * pitch:] == PAD).all())
        return out, intact


TAIL = 64  # canary bytes behind the last plane of an allocation


def plane_geometry(shapes, layouts, stacked=False):
    """Where the planes of one frame lie: -> (allocations, planes) with allocations = [size in bytes] and planes = [(allocation index, byte
    offset in it, pitch, rows, row_bytes)] in plane order.  shapes = [(rows, row_bytes)].

    stacked=False: `layouts` holds one (align, extra, offset) per plane, each plane in an allocation of its own with
    pitch = round_up(row_bytes, align) + extra and its first byte `offset` bytes in.
    stacked=True: `layouts` is ONE (align, extra, offset): every plane in the same allocation with the same
    pitch = round_up(widest row_bytes, align) + extra, plane i right behind plane i - 1's rows_{i-1} * pitch bytes — the way a contiguous
    [C, H, W] tensor and a planar surface cut from one allocation lie (equal planes: base + offset + i * rows * pitch)."""
    if stacked:
        align, extra, offset = layouts
        pitch = round_up(max(rb for _, rb in shapes), align) + extra
        planes, at = [], offset
        for rows, rb in shapes:
            planes.append((0, at, pitch, rows, rb))
            at += rows * pitch
        return [at + TAIL], planes
    assert len(layouts) == len(shapes)
    allocs, planes = [], []
    for k, ((rows, rb), (align, extra, offset)) in enumerate(zip(shapes, layouts)):
        pitch = round_up(rb, align) + extra
        planes.append((k, offset, pitch, rows, rb))
        allocs.append(offset + rows * pitch + TAIL)
    return allocs, planes


class LaidOutPlanes:
    """DevPlanes with a layout per plane: `layouts` = one (align, extra, offset) per plane, or with stacked=True ONE of them for all planes
    in one allocation (plane_geometry).  Everything that is not a pixel — row padding, the lead, the tail, the rows' padding between
    stacked planes — is 0xCD, and download() reports whether all of it still is."""

    def __init__(self, host_planes, layouts, stacked=False, device="cuda:0"):
        self.host_shapes = [(p.shape, p.dtype) for p in host_planes]
        shapes = [(p.shape[0], p.shape[1] * p.dtype.itemsize) for p in host_planes]
        self.sizes, self.planes = plane_geometry(shapes, layouts, stacked)
        self.bufs = [torch.from_numpy(h).to(device) for h in self._host_image(host_planes)]
        self.pitches = [pl[2] for pl in self.planes]

    def _host_image(self, host_planes):
        hs = [np.full((size,), PAD, dtype=np.uint8) for size in self.sizes]
        for (a, off, pitch, rows, rb), p in zip(self.planes, host_planes):
            # (the last row of a plane ends at its row bytes: the view below never reaches into the next plane or the tail)
            np.lib.stride_tricks.as_strided(hs[a][off:], shape=(rows, rb), strides=(pitch, 1))[...] = np.ascontiguousarray(p).view(np.uint8).reshape(rows, rb)
        return hs

    def desc(self):
        return [(self.bufs[a].data_ptr() + off, pitch) for a, off, pitch, _, _ in self.planes]

    def upload(self, host_planes):
        """new pixels into the SAME device buffers; the canary is renewed"""
        for b, h in zip(self.bufs, self._host_image(host_planes)):
            b.copy_(torch.from_numpy(h))

    def download(self):
        """-> (list of tight numpy planes, intact: every byte that is not a pixel still holds the canary)"""
        hs = [b.cpu().numpy().copy() for b in self.bufs]
        out = []
        for (a, off, pitch, rows, rb), (shape, dt) in zip(self.planes, self.host_shapes):
            body = np.lib.stride_tricks.as_strided(hs[a][off:], shape=(rows, rb), strides=(pitch, 1))
            out.append(body.copy().view(dt).reshape(shape))
            body[...] = PAD  # what is left over below is canary only
        return out, all(bool((h == PAD).all()) for h in hs)


def stream_handle():
    return torch.cuda.current_stream().cuda_stream


def assert_planes_equal(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            d = np.argwhere(g != w)
            first = tuple(d[0])
            raise AssertionError(
                f"{what}: plane {i} differs at {len(d)} of {g.size} elements; first at {first}: got {g[first]} want {w[first]}")
