"""Host-side mirror of the reference's SELD_evaluation_metrics.py: the segment-based, location-aware DCASE score.  The eleven counters
live on the device and seld_dcase_update (seld_amd/csrc/dcase.hip) accumulates all files of a call in one pass over the ensembled
outputs, where the reference scores a file at a time from nested dicts read back from a csv file (SELD_evaluation_metrics.py:63-154).
`compute_seld_scores` reads the eleven doubles.  `sweep_seld_scores` (seld_dcase_sweep) returns the counters of every single-class
threshold change in one call: what seld_amd/search_best.py descends on."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, utils

eps = np.finfo(float).eps
STATE_NAMES = ("TP", "FP", "FN", "S", "D", "I", "Nref", "total_DE", "DE_TP", "DE_FP", "DE_FN")


def seld_scores_from_state(state):
    """the four formulas (SELD_evaluation_metrics.py:56-61) on the eleven counters -> ER, F, LE, LR"""
    TP, FP, FN, S, D, I, Nref, total_DE, DE_TP, DE_FP, DE_FN = (float(v) for v in state)
    ER = (S + D + I) / float(Nref + eps)
    F = TP / (eps + TP + 0.5 * (FP + FN))
    LE = total_DE / float(DE_TP + eps) if DE_TP else 180
    LR = DE_TP / (eps + DE_TP + DE_FN)
    return ER, F, LE, LR


class SELDMetrics_(object):
    def __init__(self, doa_threshold=20, nb_classes=11, device=None):
        self._nb_classes, self._spatial_T = int(nb_classes), float(doa_threshold)
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SeldLibraryError("no HIP device visible: seld_amd has no CPU fallback")
        self._dev = device if isinstance(device, torch.device) else torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.state = torch.zeros(int(self.lib.seld_dcase_state_size()), dtype=torch.float64, device=self._dev)
        self._scratch = None

    def reset_states(self):
        self.state.zero_()

    def _inputs(self, pred, gt):
        """the checks and device tensors update_seld_scores and sweep_seld_scores share -> (sed, doa, gt, n_files)"""
        if isinstance(pred, (list, tuple)) and len(pred) == 2 and isinstance(pred[0], torch.Tensor):
            pred = [pred]
        pred = list(pred)
        if isinstance(gt, utils.PackedLabels):
            if len(gt.file_off) - 1 != len(pred):
                raise ValueError(f"{len(pred)} predicted files, labels of {len(gt.file_off) - 1}")
        else:
            gt = utils.concat_labels(gt)
            if len(gt.file_off) - 1 != len(pred):
                raise ValueError(f"{len(pred)} predicted files, labels of {len(gt.file_off) - 1}")
        nc = self._nb_classes
        for i, (s, d) in enumerate(pred):
            T = int(gt.file_off[i + 1] - gt.file_off[i])
            if tuple(s.shape) != (T, nc) or tuple(d.shape) != (T, 3 * nc):
                raise ValueError(f"file {i}: outputs {tuple(s.shape)}, {tuple(d.shape)} for {T} label frames of {nc} classes")
        if gt.n_classes != nc:
            raise ValueError(f"labels packed for {gt.n_classes} classes, the scorer has {nc}")
        dev = self._dev
        sed = torch.cat([torch.as_tensor(s, dtype=torch.float32, device=dev) for s, _ in pred]).contiguous()
        doa = torch.cat([torch.as_tensor(d, dtype=torch.float32, device=dev) for _, d in pred]).contiguous()
        return sed, doa, gt, len(pred)

    def _scratch_of(self, need):
        if self._scratch is None or self._scratch.numel() * 8 < need:
            self._scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=self._dev)
        return self._scratch

    def update_seld_scores(self, pred, gt, sed_thresh=0.5):
        """pred: (sed [T, nc], doa [T, 3nc]) device tensors of one file, or a list of such pairs; gt: what utils.pack_labels returned for
        that file, a list of those, or utils.concat_labels of the list (packed and uploaded once, scored many times).  A class is active
        where sed > sed_thresh (a scalar or a per-class sequence).  All files are scored in one seld_dcase_update call."""
        sed, doa, gt, n_files = self._inputs(pred, gt)
        nc, dev = self._nb_classes, self._dev
        xyz, slot, n = gt.to_device(dev)
        thr = torch.as_tensor(utils.thresh_table(sed_thresh, nc)).to(dev)
        scratch = self._scratch_of(int(self.lib.seld_dcase_update_scratch_bytes(gt.n_frames, n_files, utils.SEGMENT_FRAMES)))
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(self.lib.seld_dcase_update(sed.data_ptr(), doa.data_ptr(), thr.data_ptr(), xyz.data_ptr(), slot.data_ptr(), n.data_ptr(),
                                              gt.file_off.ctypes.data_as(C.POINTER(C.c_int32)), n_files, nc, gt.K, utils.SEGMENT_FRAMES,
                                              self._spatial_T, self.state.data_ptr(), scratch.data_ptr(), st))

    def sweep_seld_scores(self, pred, gt, base_thresh, candidates):
        """One seld_dcase_sweep call over `pred` and `gt` (as update_seld_scores takes them) -> (table float64 [nc, M, 11], base float64 [11]),
        numpy: table[c, k] holds the counters update_seld_scores would leave in a fresh state for `base_thresh` (a scalar or a per-class
        sequence) with class c's entry replaced by candidates[k], bit for bit; `base` those of base_thresh itself.  self.state is not touched."""
        sed, doa, gt, n_files = self._inputs(pred, gt)
        nc, dev = self._nb_classes, self._dev
        cand = np.ascontiguousarray(np.asarray(candidates, np.float32).reshape(-1))
        M = int(cand.size)
        need = int(self.lib.seld_dcase_sweep_scratch_bytes(gt.n_frames, n_files, nc, M, utils.SEGMENT_FRAMES))
        if need < 0:
            raise ValueError(f"sweep_seld_scores: {M} candidates (1..16 are swept at once), or outputs past 32-bit indexing")
        xyz, slot, n = gt.to_device(dev)
        thr = torch.as_tensor(utils.thresh_table(base_thresh, nc)).to(dev)
        cand_d = torch.as_tensor(cand).to(dev)
        table = torch.empty((nc * M + 1, self.state.numel()), dtype=torch.float64, device=dev)
        scratch = self._scratch_of(need)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(self.lib.seld_dcase_sweep(sed.data_ptr(), doa.data_ptr(), thr.data_ptr(), cand_d.data_ptr(), xyz.data_ptr(), slot.data_ptr(),
                                             n.data_ptr(), gt.file_off.ctypes.data_as(C.POINTER(C.c_int32)), n_files, nc, gt.K, M,
                                             utils.SEGMENT_FRAMES, self._spatial_T, table.data_ptr(), scratch.data_ptr(), st))
        out = table.cpu().numpy()
        return out[:-1].reshape(nc, M, -1), out[-1].copy()

    def counters(self) -> dict:
        return dict(zip(STATE_NAMES, self.state.cpu().numpy().tolist()))

    def compute_seld_scores(self):
        """-> ER, F, LE, LR (SELD_evaluation_metrics.py:48-61)"""
        return seld_scores_from_state(self.state.cpu().numpy())


def early_stopping_metric(sed_error, doa_error):
    """SELD_evaluation_metrics.py:223-237: mean of ER, 1 - F, LE / 180 and 1 - LR"""
    return np.mean([sed_error[0], 1 - sed_error[1], doa_error[0] / 180, 1 - doa_error[1]])
