"""Host-side mirror of the DCASE answer-file helpers of the reference's utils.py: write_answer (utils.py:249-268),
load_output_format_file (:271-291), segment_labels (:293-324), convert_output_format_cartesian_to_polar (:327-340) and
convert_output_format_polar_to_cartesian (:352-367), plus `pack_labels`, which lays a label dict out as the arrays that
seld_dcase_update reads.  The rows of an answer file are chosen and gathered on the device (seld_answer_rows); only the active rows come
to the host to be formatted."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

SEGMENT_FRAMES = 10          # segment_labels' block length (utils.py:294-296)
MAX_SLOTS = 8                # SELD_DCASE_MAX_SLOTS


def load_output_format_file(_output_format_file):
    """DCASE output-format csv -> {frame: [[class, azimuth, elevation, track]]} for 5-word lines (polar) or
    {frame: [[class, x, y, z, track]]} for 6-word lines (cartesian), as utils.py:271-291 reads them."""
    out = {}
    with open(_output_format_file, 'r') as fid:
        for line in fid:
            words = line.strip().split(',')
            frame = int(float(words[0]))
            if len(words) == 5:
                row = [int(float(words[1])), float(words[3]), float(words[4]), int(float(words[2]))]
            elif len(words) == 6:
                row = [int(float(words[1])), float(words[3]), float(words[4]), float(words[5]), int(float(words[2]))]
            else:
                continue
            out.setdefault(frame, []).append(row)
    return out


def segment_labels(_pred_dict, _max_frames):
    """{frame: rows} -> {segment: {class: [[frames in the segment], [[row[1:], ...] per frame]]]}} over ceil(_max_frames / 10) segments
    (utils.py:293-324)."""
    nb_blocks = int(np.ceil(_max_frames / float(SEGMENT_FRAMES)))
    output_dict = {x: {} for x in range(nb_blocks)}
    for frame_cnt in range(0, _max_frames, SEGMENT_FRAMES):
        block_cnt = frame_cnt // SEGMENT_FRAMES
        loc_dict = {}
        for audio_frame in range(frame_cnt, frame_cnt + SEGMENT_FRAMES):
            for value in _pred_dict.get(audio_frame, ()):
                loc_dict.setdefault(value[0], {}).setdefault(audio_frame - frame_cnt, []).append(value[1:])
        for class_cnt, frames in loc_dict.items():
            output_dict[block_cnt].setdefault(class_cnt, []).append([list(frames.keys()), list(frames.values())])
    return output_dict


def convert_output_format_polar_to_cartesian(in_dict):
    out_dict = {}
    for frame_cnt, rows in in_dict.items():
        out_dict[frame_cnt] = []
        for v in rows:
            ele_rad = v[2] * np.pi / 180.
            azi_rad = v[1] * np.pi / 180
            tmp_label = np.cos(ele_rad)
            out_dict[frame_cnt].append([v[0], np.cos(azi_rad) * tmp_label, np.sin(azi_rad) * tmp_label, np.sin(ele_rad), v[-1]])
    return out_dict


def convert_output_format_cartesian_to_polar(in_dict):
    out_dict = {}
    for frame_cnt, rows in in_dict.items():
        out_dict[frame_cnt] = []
        for v in rows:
            x, y, z = v[1], v[2], v[3]
            azimuth = np.arctan2(y, x) * 180 / np.pi
            elevation = np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) * 180 / np.pi
            out_dict[frame_cnt].append([v[0], azimuth, elevation, v[-1]])
    return out_dict


class PackedLabels:
    """The ground truth of one or more files as seld_dcase_update reads it: xyz [N, nc, K, 3] float64, slot [N, nc, K] uint8,
    n [N, nc] int32 and file_off [n_files + 1] int32 (numpy, on the host).  `to_device` uploads the three arrays once per device."""

    def __init__(self, xyz, slot, n, file_off):
        self.xyz, self.slot, self.n = xyz, slot, n
        self.file_off = np.ascontiguousarray(file_off, np.int32)
        self._dev = {}

    @property
    def K(self) -> int:
        return int(self.xyz.shape[2])

    @property
    def n_classes(self) -> int:
        return int(self.n.shape[1])

    @property
    def n_frames(self) -> int:
        return int(self.n.shape[0])

    def to_device(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.as_tensor(np.ascontiguousarray(a)).to(device) for a in (self.xyz, self.slot, self.n))
        return self._dev[key]


def pack_labels(label_dict, n_frames, n_classes):
    """A cartesian label dict ({frame: [[class, x, y, z, track], ...]}: what convert_output_format_polar_to_cartesian returns) of one file
    with `n_frames` predicted label frames -> PackedLabels.  K is the largest number of same-class entries in one frame (at least 1).  An
    entry's slot is the index of its track id among the distinct ids of its (10-frame segment, class), in order of first appearance: frames
    ascending, entries in file order.  Frames >= n_frames are dropped, and so are classes outside 0..n_classes-1, which the scorer's
    `range(nb_classes)` never visits (SELD_evaluation_metrics.py:75).  ValueError for more than 8 same-class entries in a frame or more than
    8 distinct track ids in a (segment, class)."""
    n_frames, n_classes = int(n_frames), int(n_classes)
    if n_frames < 1 or n_classes < 1:
        raise ValueError("pack_labels: n_frames and n_classes must be positive")
    per = {}
    for frame in sorted(label_dict):
        if not 0 <= frame < n_frames:
            continue
        for row in label_dict[frame]:
            if len(row) != 5:
                raise ValueError("pack_labels takes cartesian rows [class, x, y, z, track] (convert_output_format_polar_to_cartesian)")
            c = int(row[0])
            if 0 <= c < n_classes:
                per.setdefault((frame, c), []).append(row)
    K = max([len(v) for v in per.values()], default=1)
    if K > MAX_SLOTS:
        raise ValueError(f"pack_labels: {K} same-class entries in one frame, at most {MAX_SLOTS} are packed")
    xyz = np.zeros((n_frames, n_classes, K, 3), np.float64)
    slot = np.zeros((n_frames, n_classes, K), np.uint8)
    n = np.zeros((n_frames, n_classes), np.int32)
    ids = {}
    for (frame, c), rows in per.items():            # insertion order: frames ascending
        seen = ids.setdefault((frame // SEGMENT_FRAMES, c), [])
        for e, row in enumerate(rows):
            track = row[4]
            if track not in seen:
                seen.append(track)
                if len(seen) > MAX_SLOTS:
                    raise ValueError(f"pack_labels: more than {MAX_SLOTS} distinct track ids of class {c} in segment {frame // SEGMENT_FRAMES}")
            xyz[frame, c, e] = row[1:4]
            slot[frame, c, e] = seen.index(track)
        n[frame, c] = len(rows)
    return PackedLabels(xyz, slot, n, [0, n_frames])


def concat_labels(packed):
    """[PackedLabels of one file each, ...] -> one PackedLabels over all of them (K = the largest; file_off from the frame counts)"""
    packed = list(packed)
    if not packed:
        raise ValueError("concat_labels: no files")
    nc = packed[0].n_classes
    if any(p.n_classes != nc for p in packed):
        raise ValueError("concat_labels: the files differ in n_classes")
    K = max(p.K for p in packed)
    N = sum(p.n_frames for p in packed)
    xyz = np.zeros((N, nc, K, 3), np.float64)
    slot = np.zeros((N, nc, K), np.uint8)
    off, t = [0], 0
    for p in packed:
        if len(p.file_off) != 2:
            raise ValueError("concat_labels takes single-file labels")
        xyz[t:t + p.n_frames, :, :p.K] = p.xyz
        slot[t:t + p.n_frames, :, :p.K] = p.slot
        t += p.n_frames
        off.append(t)
    return PackedLabels(xyz, slot, np.concatenate([p.n for p in packed]), off)


def thresh_table(sed_thresh, n_classes):
    """a scalar or a per-class sequence -> float32 [n_classes]"""
    t = np.asarray(sed_thresh, np.float32).reshape(-1)
    if t.size == 1:
        t = np.full(n_classes, t[0], np.float32)
    if t.size != n_classes:
        raise ValueError(f"sed_thresh has {t.size} entries for {n_classes} classes")
    return np.ascontiguousarray(t)


def answer_rows(sed, doa, sed_thresh, file_off):
    """seld_answer_rows on concatenated device tensors sed [N, nc], doa [N, 3nc] -> (row_fc int32 [cap, 2], row_xyz float32 [cap, 3],
    row_off int32 [n_files + 1]) on the device; file f's rows are row_fc[row_off[f]:row_off[f + 1]]."""
    import torch
    lib = _lib.load()
    if not (isinstance(sed, torch.Tensor) and sed.is_cuda and isinstance(doa, torch.Tensor) and doa.is_cuda):
        raise _lib.SeldLibraryError("answer rows are chosen on the device: sed and doa must be device tensors (seld_amd has no CPU fallback)")
    sed = sed.to(torch.float32).contiguous()
    doa = doa.to(torch.float32).contiguous()
    N, nc = sed.shape
    file_off = np.ascontiguousarray(file_off, np.int32)
    if tuple(doa.shape) != (N, 3 * nc) or file_off.ndim != 1 or file_off.size < 2 or int(file_off[-1]) != N:
        raise ValueError("answer_rows: sed [N, nc], doa [N, 3nc], file_off[-1] = N")
    n_files = file_off.size - 1
    dev = sed.device
    thr = torch.as_tensor(thresh_table(sed_thresh, nc)).to(dev)
    need = int(lib.seld_answer_rows_scratch_bytes(N, n_files, nc))
    if need < 0:
        raise ValueError("answer_rows: N * nc does not fit 32 bits")
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    row_fc = torch.empty((N * nc, 2), dtype=torch.int32, device=dev)
    row_xyz = torch.empty((N * nc, 3), dtype=torch.float32, device=dev)
    row_off = torch.empty(n_files + 1, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.seld_answer_rows(sed.data_ptr(), doa.data_ptr(), thr.data_ptr(), file_off.ctypes.data_as(C.POINTER(C.c_int32)), n_files, nc,
                                    row_fc.data_ptr(), row_xyz.data_ptr(), row_off.data_ptr(), scratch.data_ptr(), st))
    return row_fc, row_xyz, row_off


def format_answer_rows(row_fc, row_xyz) -> str:
    """the text of utils.write_answer (utils.py:267-268): frame, class, track 0 and float() of the three float32 values, whose repr reads
    back to the same float32"""
    return "".join('{},{},{},{},{},{}\n'.format(int(fc[0]), int(fc[1]), 0, float(v[0]), float(v[1]), float(v[2]))
                   for fc, v in zip(np.asarray(row_fc), np.asarray(row_xyz, np.float32)))


def write_answer(output_dir, filename, preds, direction):
    """utils.write_answer (utils.py:249-268): one csv row per active (frame, class) of `preds` (a boolean or thresholded [T, nc] device
    tensor), row-major, with `direction[t, c::nc]` ([T, 3nc], device) beside it.  The rows are compacted on the device and only they are
    copied to the host.  Where no class is ever active the reference raises (tf.stack of an empty list); here an empty file is written."""
    import torch
    if not (isinstance(preds, torch.Tensor) and preds.is_cuda):
        raise _lib.SeldLibraryError("write_answer takes device tensors (seld_amd has no CPU fallback)")
    row_fc, row_xyz, row_off = answer_rows(preds.to(torch.float32), direction, 0.5, [0, int(preds.shape[0])])
    n = int(row_off[1].item())
    text = format_answer_rows(row_fc[:n].cpu().numpy(), row_xyz[:n].cpu().numpy())
    with open(os.path.join(output_dir, filename), 'w') as fid:
        fid.write(text)
