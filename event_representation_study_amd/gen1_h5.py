"""The event side of the reference's Gen1 container (ev-YOLOv6/yolov6/data/gen1_2yolo.py:72-82,150-198): one HDF5 group per
recording, ``<name>/events/{x, y, t, p, height, width}`` and ``<name>/bbox/{t_unique, event_idx, ...}``; sample ``idx`` is the
window of the ``num_events`` events in front of the idx-th labelled timestamp of the recordings taken in name order
(``convert_idx_to_rel_idx``, ``_load_bbox``: event_idx; ``_load_events``: [max(0, event_idx - num_events), event_idx), t rebased
to the window's first event).  Read with h5lite -- chunk-wise, Blosc included -- so a window costs its own chunks, not the
recording.  ``windows(indices)`` hands (n, 4) int32 arrays to ``EventBatch.from_numpy`` / the precompute pipeline;
``device_windows(indices)`` uploads the touched span of every recording once and cuts the same windows on the device."""
import numpy as np

from .synthetic import int64_to_int32

from . import h5lite


class Gen1H5Events:
    def __init__(self, path, num_events=50000):
        self.h5 = h5lite.File(str(path))
        self.num_events = int(num_events)
        self._file_names = sorted(self.h5.keys())                                              # :77
        self._num_unique_bboxes = [len(self.h5["%s/bbox/t_unique" % f]) for f in self._file_names]   # :78-80
        first = self._file_names[0]
        self.height = int(self.h5["%s/events/height" % first][()])                             # :82-83
        self.width = int(self.h5["%s/events/width" % first][()])
        self._event_idx = {}
        self._device = {}       # recording name -> (first event of the uploaded span, DeviceRecording): device_windows' cache

    def __len__(self):
        return int(sum(self._num_unique_bboxes))

    def locate(self, idx):
        """(index inside its recording, recording name): convert_idx_to_rel_idx, :158-166"""
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        counter = 0
        while idx >= self._num_unique_bboxes[counter]:
            idx -= self._num_unique_bboxes[counter]
            counter += 1
        return idx, self._file_names[counter]

    def _range(self, name, rel):
        """[idx0, idx1) of the rel-th label of a recording: the num_events events in front of its event_idx, :186-190"""
        if name not in self._event_idx:
            self._event_idx[name] = np.asarray(self.h5["%s/bbox/event_idx" % name][:]).astype(np.int64)
        idx1 = int(self._event_idx[name][rel])
        return max(0, idx1 - self.num_events), idx1

    def window(self, idx):
        """(n, 4) int32 rows [x, y, t - t[0], p] of sample idx (_load_bbox's event_idx, _load_events)."""
        rel, name = self.locate(idx)
        idx0, idx1 = self._range(name, rel)
        ev = self.h5["%s/events" % name]
        x, y, t, p = (np.asarray(ev[k][idx0:idx1]) for k in ("x", "y", "t", "p"))
        if idx1 - idx0 <= 0:
            raise IndexError("sample %d: no events before its label (the reference fails on xyt[0, -1], gen1_2yolo.py:196)" % idx)
        out = np.empty((idx1 - idx0, 4), dtype=np.int32)
        # range-checked narrowing: a corrupt container (or a window of more than 2^31 us) fails loudly instead of wrapping
        out[:, 0], out[:, 1], out[:, 3] = (int64_to_int32(np.asarray(v).astype(np.int64), n) for v, n in ((x, "x"), (y, "y"), (p, "p")))
        out[:, 2] = int64_to_int32(t.astype(np.int64) - int(t[0]), "t")                         # xyt[:, -1] -= xyt[0, -1], :196
        return out

    def windows(self, indices):
        return [self.window(int(i)) for i in indices]

    def device_windows(self, indices, device="cuda:0"):
        """The samples ``indices`` as ONE EventBatch, in that order, cut on the device: ``events`` and ``offsets`` equal
        ``EventBatch.from_numpy(self.windows(indices), height, width)``.  The samples are grouped by recording; the span of
        events a recording's samples touch is read and uploaded once and kept (a dict per recording; a later call that
        reaches outside the kept span uploads the union), so overlapping windows -- consecutive labels share most of theirs --
        cross PCIe once.  Samples of several recordings are gathered from the device-side concatenation of the kept spans."""
        from .recording import DeviceRecording
        where = [self.locate(int(i)) for i in indices]
        ranges = [self._range(name, rel) for rel, name in where]
        for k, (a, e) in enumerate(ranges):
            if e - a <= 0:
                raise IndexError("sample %d: no events before its label (the reference fails on xyt[0, -1], gen1_2yolo.py:196)"
                                 % int(indices[k]))
        names = sorted({name for _, name in where})
        for name in names:
            lo = min(a for (a, _), (_, nm) in zip(ranges, where) if nm == name)
            hi = max(e for (_, e), (_, nm) in zip(ranges, where) if nm == name)
            kept = self._device.get((name, str(device)))
            if kept is not None:
                if kept[0] <= lo and hi <= kept[0] + len(kept[1]):
                    continue
                lo, hi = min(lo, kept[0]), max(hi, kept[0] + len(kept[1]))
            ev = self.h5["%s/events" % name]
            x, y, t, p = (np.asarray(ev[k][lo:hi]) for k in ("x", "y", "t", "p"))
            self._device[(name, str(device))] = (lo, DeviceRecording(x, y, t, p, self.height, self.width, device=device))
        kept = [self._device[(name, str(device))] for name in names]
        if len(kept) == 1:
            rec, shift = kept[0][1], {names[0]: -kept[0][0]}
        else:       # one gather over the spans laid end to end (device-to-device copies of the columns)
            starts = np.concatenate([[0], np.cumsum([len(r) for _, r in kept])])
            shift = {name: int(s) - lo for name, s, (lo, _) in zip(names, starts, kept)}
            rec = DeviceRecording.concatenated([r for _, r in kept])
        i0 = np.array([a + shift[nm] for (a, _), (_, nm) in zip(ranges, where)], np.int64)
        i1 = np.array([e + shift[nm] for (_, e), (_, nm) in zip(ranges, where)], np.int64)
        return rec.windows(i0, i1, rebase="first")
