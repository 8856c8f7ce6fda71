"""The training set resident in device memory, and batches collated there (csrc/collate.hip).

`ResidentSet` reads every utterance ONCE through `DaftExprtDataLoader.__getitem__` (the seeded list shuffle and the float64
standardisation with preserved zeros are therefore the loader's own bits), packs the arrays back to back and uploads them.
`ResidentLoader` stands in for the `DataLoader`: batch composition still comes from torch's sampler classes iterated on the host,
but an epoch's index lists are uploaded once and every batch is two kernel launches (`dx_collate_order`, `dx_collate_gather`)
that replace `DaftExprtDataCollate` (the reference's `data_loader.py:146-211`) and the per-step H2D copy.  Nothing during an epoch
copies from the device or synchronises.  Opt-in (`hparams.resident_data_set`); a feeder of the train loop like `data_loader.HostUnits`.
"""
import logging
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
from torch.utils.data.distributed import DistributedSampler

from daft_exprt import _hip as H
from daft_exprt.data_loader import DaftExprtDataLoader, GroupedBatch, check_group_sizes, prepare_data_loaders, take_groups

_logger = logging.getLogger(__name__)

MAX_BATCH = int(H.lib().dx_collate_max_batch())     # utterances of one micro-batch (the order kernel's LDS capacity)
GATHER_SPAN = int(H.lib().dx_collate_span())        # positions of one output row per workgroup of the gather kernel
_SYM_ARRAYS = (('sym', torch.int32), ('dur_f', torch.float32), ('dur_i', torch.int32), ('sym_en', torch.float32),
               ('sym_pi', torch.float32))           # items[0..4]
_FRM_ARRAYS = (('frm_en', torch.float32), ('frm_pi', torch.float32))   # items[5..6]


def stable_order(lengths):
    ''' positions of a batch ordered by length, descending and STABLE (ties keep the sampler's order): the row order
        `dx_collate_order` produces.  (`torch.sort(descending=True)` of the host collate does not keep ties in order.) '''
    return np.argsort(-np.asarray(lengths, dtype=np.int64), kind='stable')


def packed_bytes(L, T, n_mel):
    ''' size of the packed store for these per-utterance symbol / frame counts '''
    L, T = np.asarray(L, dtype=np.int64), np.asarray(T, dtype=np.int64)
    return int(L.sum()) * 4 * len(_SYM_ARRAYS) + int(T.sum()) * 4 * (len(_FRM_ARRAYS) + n_mel) + 8 * (3 * len(L) + 2)


def list_bytes(list_file, hparams):
    ''' packed size of a list file's utterances WITHOUT reading their data: T from the `.npy` header, L = the lines of `.markers` '''
    L, T = [], []
    with open(list_file, 'r', encoding='utf-8') as f:
        for line in f:
            if line.strip():
                features_dir, feature_file = line.strip().split('|')[:2]
                base = os.path.join(features_dir, feature_file)
                T.append(np.load(base + '.npy', mmap_mode='r').shape[1])
                with open(base + '.markers', 'r', encoding='utf-8') as m:
                    L.append(sum(1 for _ in m))
    return packed_bytes(L, T, hparams.n_mel_channels)


class ResidentBatch(tuple):
    ''' the 13-tuple `DaftExprt.parse_batch` takes (device tensors, then the host lists of dirs and files in row order), plus
        `.frames` = sum(T) as a host int, `.order` = the position in the sampler's batch of each row (host list) and
        `.device_order` = the same as the order kernel wrote it (int64 device tensor) '''
    def __new__(cls, fields, frames, order, device_order):
        self = super().__new__(cls, fields)
        self.frames, self.order, self.device_order = frames, order, device_order
        return self


class ResidentSet(object):
    ''' the packed store (layout: include/daft_exprt_hip.h, K26).  Tensors on `device`: sym, dur_f, dur_i, sym_en, sym_pi (sum L),
        frm_en, frm_pi (sum T), mel (n_mel * sum T), sym_off, frm_off (U + 1) int64, speaker (U) int64.  Host copies (numpy): L, T,
        sym_off_host, frm_off_host; `dirs` / `files` lists; `index` = the position in the list file of every utterance held, out of
        `n_global`. '''
    def __init__(self, items, hparams, device, index=None, n_global=None):
        from daft_exprt.model import DaftExprt
        assert len(items) > 0, 'ResidentSet: no utterances'
        self.device = torch.device(device)
        self.n_mel = int(hparams.n_mel_channels)
        self.L = np.array([len(it[0]) for it in items], dtype=np.int64)
        self.T = np.array([it[7].shape[1] for it in items], dtype=np.int64)
        for it, l, t in zip(items, self.L, self.T):
            assert it[7].shape[0] == self.n_mel and all(len(it[k]) == l for k in range(5)) and len(it[5]) == t == len(it[6])
        self.sym_off_host = np.concatenate(([0], np.cumsum(self.L)))
        self.frm_off_host = np.concatenate(([0], np.cumsum(self.T)))
        self.dirs, self.files = [it[9] for it in items], [it[10] for it in items]
        self.index = np.arange(len(items), dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
        self.local_of = {int(g): i for i, g in enumerate(self.index)}
        self.n_global = int(n_global) if n_global is not None else int(self.index.max()) + 1    # utterances of the whole list
        self.nbytes = packed_bytes(self.L, self.T, self.n_mel)
        pin = self.device.type == 'cuda'
        stage = lambda n, dtype: torch.empty(n, dtype=dtype, pin_memory=pin)
        host = {}
        for k, (name, dtype) in enumerate(_SYM_ARRAYS):
            host[name] = stage(int(self.sym_off_host[-1]), dtype)
            host[name].copy_(torch.cat([it[k].reshape(-1) for it in items]))
        for k, (name, dtype) in enumerate(_FRM_ARRAYS):
            host[name] = stage(int(self.frm_off_host[-1]), dtype)
            host[name].copy_(torch.cat([it[5 + k].reshape(-1) for it in items]))
        host['mel'] = stage(self.n_mel * int(self.frm_off_host[-1]), torch.float32)
        for it, f0, t in zip(items, self.frm_off_host, self.T):     # each utterance as its .npy file is: (n_mel, T_u) row-major
            host['mel'][self.n_mel * f0:self.n_mel * (f0 + t)].view(self.n_mel, t).copy_(it[7])
        host['sym_off'], host['frm_off'] = torch.from_numpy(self.sym_off_host), torch.from_numpy(self.frm_off_host)
        host['speaker'] = torch.tensor([int(it[8]) for it in items], dtype=torch.int64)
        # DaftExprt.check_ids' range checks, once over the whole set (device batches pass parse_batch unchecked)
        DaftExprt.check_ids(SimpleNamespace(hp=hparams), host['sym'], host['speaker'], training=True)
        for name, t in host.items():
            setattr(self, name, t.to(self.device, non_blocking=True) if pin else t)
        if pin:
            torch.cuda.synchronize(self.device)       # the staging buffers go away with `host`

    @classmethod
    def from_items(cls, items, hparams, device, index=None, n_global=None):
        ''' items: sequences in the order of `DaftExprtDataLoader.__getitem__` / `SyntheticUtterances.__getitem__` '''
        return cls(list(items), hparams, device, index=index, n_global=n_global)

    @classmethod
    def from_list(cls, list_file, hparams, device, shuffle=True, indices=None):
        ''' the utterances `indices` (default: all) of the list file, numbered as `DaftExprtDataLoader(list_file, hparams, shuffle)`
            numbers them (after its seeded shuffle) '''
        ds = DaftExprtDataLoader(list_file, hparams, shuffle=shuffle)
        indices = list(range(len(ds))) if indices is None else [int(i) for i in indices]
        with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as ex:
            items = list(ex.map(ds.__getitem__, indices))
        return cls(items, hparams, device, index=indices, n_global=len(ds))

    def __len__(self):
        return len(self.L)

    def item(self, u):
        ''' utterance u back out of the packed arrays (host tensors), in the order of `__getitem__` '''
        s0, s1, f0, f1 = self.sym_off_host[u], self.sym_off_host[u + 1], self.frm_off_host[u], self.frm_off_host[u + 1]
        sym = [getattr(self, name)[s0:s1].cpu() for name, _ in _SYM_ARRAYS]
        frm = [getattr(self, name)[f0:f1].cpu() for name, _ in _FRM_ARRAYS]
        mel = self.mel[self.n_mel * f0:self.n_mel * f1].cpu().view(self.n_mel, f1 - f0)
        return sym + frm + [mel, int(self.speaker[u]), self.dirs[u], self.files[u]]


class _Unit(object):
    ''' one yield of the loader as the host plans it: `micro` = the local utterance indices of each micro-batch '''
    def __init__(self, rset, micro):
        self.micro = [np.asarray(m, dtype=np.int64) for m in micro]
        self.sizes = [len(m) for m in self.micro]
        self.pads = np.array([[rset.L[m].max(), rset.T[m].max()] for m in self.micro], dtype=np.int64)   # (L_pad, T_pad) each
        self.L_pad, self.T_pad = int(self.pads[:, 0].max()), int(self.pads[:, 1].max())
        order = [stable_order(rset.L[m]) for m in self.micro]
        self.order = [int(p) for o in order for p in o]
        rows = np.concatenate([m[o] for m, o in zip(self.micro, order)])
        self.frames = int(rset.T[rows].sum())
        self.dirs, self.files = [rset.dirs[u] for u in rows], [rset.files[u] for u in rows]


class ResidentLoader(object):
    ''' iterable with `__len__`, like the `DataLoader` it stands in for.  Batch composition: `BatchSampler` over `RandomSampler`
        (shuffle), `SequentialSampler` (not), or `DistributedSampler(shuffle=False)` of `distributed = (world, rank)` over the WHOLE
        list -- the set then holds that rank's shard (`ResidentSet.index`).  group = accum > 1 yields `accum` consecutive
        micro-batches as one `GroupedBatch`; an incomplete group at the end of an epoch is carried into the next one.
        The launches go to `self.stream` when it is set, to the current stream otherwise. '''
    def __init__(self, rset, batch_size, shuffle=False, drop_last=False, distributed=None, group=1, stream=None):
        assert 0 < batch_size
        self.set, self.batch_size, self.drop_last, self.group, self.stream = rset, int(batch_size), bool(drop_last), max(1, int(group)), stream
        if distributed is not None:
            world, rank = distributed
            self.sampler = DistributedSampler(range(rset.n_global), num_replicas=world, rank=rank, shuffle=False)
        else:
            self.sampler = RandomSampler(range(len(rset))) if shuffle else SequentialSampler(range(len(rset)))
        self.distributed = distributed is not None
        self.batch_sampler = BatchSampler(self.sampler, self.batch_size, self.drop_last)
        self.held = []        # micro-batches (local indices) of an unfinished group, carried over the epoch boundary

    def index_lists(self):
        ''' one epoch's batches in the sampler's numbering (draws from torch's generator when shuffling) '''
        return [list(b) for b in self.batch_sampler]

    def plan_epoch(self):
        ''' [[micro-batch (local indices), ...] per yield] of the next epoch; updates `held` '''
        lists = [[self.set.local_of[int(g)] for g in b] if self.distributed else b for b in self.index_lists()]      # (a shard: local numbers)
        plan, self.held = take_groups(self.held, lists, self.group)
        return plan

    def __len__(self):
        ''' yields of the NEXT epoch (with a group, what is carried over counts) '''
        return (len(self.held) + len(self.batch_sampler)) // self.group

    def __iter__(self):
        return self._run(self.plan_epoch())

    def units(self, model, gpu):
        ''' an epoch as the train loop's feeder (`data_loader.HostUnits`); `parse_batch` launches nothing: device tensors pass through '''
        for batch in self:
            yield (batch if self.group > 1 else model.parse_batch(gpu, batch)[:2]), batch.frames

    def collate(self, micro):
        ''' these micro-batches (lists of the set's own utterance numbers; `group` of them, one without a group) as one yield, now '''
        assert len(micro) == self.group
        return next(self._run([[list(m) for m in micro]]))

    def _run(self, plan):
        units = [_Unit(self.set, micro) for micro in plan]
        if not units:
            return
        for u in units:
            assert max(u.sizes) <= MAX_BATCH, f'batch of {max(u.sizes)} utterances: dx_collate_order takes at most {MAX_BATCH}'
            check_group_sizes(u.sizes)
        dev = self.set.device
        with torch.cuda.stream(self.stream):        # (None: the current stream)
            # the epoch's index lists and padded lengths: ONE upload
            idx = np.concatenate([m for u in units for m in u.micro])
            pads = np.concatenate([u.pads.reshape(-1) for u in units])
            staged = torch.from_numpy(np.concatenate((idx, pads))).pin_memory()
            epoch = staged.to(dev, non_blocking=True)
        row, mb = 0, len(idx)
        for u in units:
            with torch.cuda.stream(self.stream):        # (None: the current stream)
                batch = self._launch(u, epoch[row:], epoch[mb:])
            row, mb = row + sum(u.sizes), mb + 2 * len(u.sizes)
            yield batch

    def _launch(self, u, idx, pads):
        from daft_exprt import ops
        s, dev = self.set, self.set.device
        n_micro, B = len(u.sizes), u.sizes[0]
        B_tot, grouped = n_micro * B, self.group > 1
        meta = ops._empty(9 if grouped else 5, B_tot, dtype=torch.int64, device=dev)
        src_utt, src_pos, in_len, out_len, spk = meta[0], meta[1], meta[2], meta[3], meta[4]
        bounds = (meta[5], meta[6], meta[7], meta[8]) if grouped else (None,) * 4
        lib, st = H.lib(), H.stream()
        H.check(lib.dx_collate_order(H.ptr(idx), H.ptr(s.sym_off), H.ptr(s.frm_off), H.ptr(s.speaker), len(s), H.ptr(pads), H.ptr(src_utt),
                                     H.ptr(src_pos), H.ptr(in_len), H.ptr(out_len), H.ptr(spk), *(H.ptr(t) for t in bounds), n_micro, B, st))
        e = lambda *shape, dtype=torch.float32: ops._empty(*shape, dtype=dtype, device=dev)
        L, T = u.L_pad, u.T_pad
        o_sym, o_dur_i = e(B_tot, L, dtype=torch.int64), e(B_tot, L, dtype=torch.int64)
        o_dur_f, o_sym_en, o_sym_pi = e(B_tot, L), e(B_tot, L), e(B_tot, L)
        o_frm_en, o_frm_pi, o_mel = e(B_tot, T), e(B_tot, T), e(B_tot, s.n_mel, T)
        H.check(lib.dx_collate_gather(H.ptr(src_utt), H.ptr(s.sym_off), H.ptr(s.frm_off), len(s), H.ptr(s.sym), H.ptr(s.dur_f), H.ptr(s.dur_i),
                                      H.ptr(s.sym_en), H.ptr(s.sym_pi), H.ptr(s.frm_en), H.ptr(s.frm_pi), H.ptr(s.mel), H.ptr(o_sym),
                                      H.ptr(o_dur_f), H.ptr(o_dur_i), H.ptr(o_sym_en), H.ptr(o_sym_pi), H.ptr(o_frm_en), H.ptr(o_frm_pi),
                                      H.ptr(o_mel), B_tot, L, T, s.n_mel, st))
        inputs = (o_sym, o_dur_f, o_dur_i, o_sym_en, o_sym_pi, in_len, o_frm_en, o_frm_pi, o_mel, out_len, spk)
        if not grouped:
            return ResidentBatch(inputs + (u.dirs, u.files), u.frames, u.order, src_pos)
        targets = (inputs[1], inputs[3], inputs[4], inputs[8], inputs[10])        # the views parse_batch hands out
        g = GroupedBatch(inputs, targets, bounds, n_micro, list(u.sizes))
        g.frames, g.order, g.device_order, g.dirs, g.files = u.frames, u.order, src_pos, u.dirs, u.files
        return g


def _list_len(list_file):
    with open(list_file, 'r', encoding='utf-8') as f:
        return sum(1 for line in f if line.strip())


def prepare_resident_loaders(hparams, device, distributed=None, group=1):
    ''' (train_loader, sampler, val_loader, n_examples) like `prepare_data_loaders`, from sets resident on `device`: the training
        loader shuffles, or -- distributed -- walks this rank's `DistributedSampler(shuffle=False)` shard, `drop_last=True`; the
        validation loader holds the whole set on every rank, in order, `drop_last=False`, `group=1`.  A set whose packed size is
        above `hparams.resident_max_bytes` logs one warning and gets the ordinary `DataLoader`s. '''
    if distributed is None:
        distributed = torch.distributed.is_available() and torch.distributed.is_initialized()
    limit = int(getattr(hparams, 'resident_max_bytes', 32 * 1024 ** 3))
    need = list_bytes(hparams.training_files, hparams) + list_bytes(hparams.validation_files, hparams)
    if need > limit:
        _logger.warning(f'resident data set: {need:_} bytes packed, above resident_max_bytes = {limit:_} -- using the DataLoader')
        return prepare_data_loaders(hparams, num_workers=8, distributed=distributed)
    n = _list_len(hparams.training_files)
    shard, indices = None, None
    if distributed:
        shard = (torch.distributed.get_world_size(), torch.distributed.get_rank())
        indices = sorted(set(DistributedSampler(range(n), num_replicas=shard[0], rank=shard[1], shuffle=False)))
    train_set = ResidentSet.from_list(hparams.training_files, hparams, device, indices=indices)
    val_set = ResidentSet.from_list(hparams.validation_files, hparams, device)
    train_loader = ResidentLoader(train_set, hparams.batch_size, shuffle=not distributed, drop_last=True, distributed=shard, group=group)
    val_loader = ResidentLoader(val_set, hparams.batch_size, shuffle=False, drop_last=False)
    _logger.info(f'resident data set: {len(train_set)} + {len(val_set)} utterances, {train_set.nbytes + val_set.nbytes:_} bytes on {device}')
    return train_loader, (train_loader.sampler if distributed else None), val_loader, n
