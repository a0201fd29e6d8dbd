"""The one cache of packed weights (BatchNorm-folded, device-layout copies) and the one rule for when a pack is stale.

A module that launches with packed weights keeps them in ONE attribute, ``__dict__[PACKED]``: a dict of named slots (``"conv"``, ``"stem"``,
``"proto_out"``, ``"block"``, ``"tail"``, ``"front"``, ``("first", level)``, ``"stem2"``).  ``packed(owner, slot, sources, dtype, device,
build)`` returns the slot's pack, building it when there is none that is still valid.  A pack is valid while

(a) ``(data_ptr, _version)`` of EVERY parameter and buffer of every source module is what it was when the slot was filled (re-homed
    storage, ``load_state_dict``, in-place edits) — a change empties the slot, all variants.  (The slot keeps the list of tensor objects
    instead of walking the modules at every call; any ``_apply`` on the owner makes it walk them again);
(b) the variant key is equal: dtype, device, the caller's extras, and everything that is not a tensor but changes the fold —
    ``H.scaled_domain()``, ``H.fp8_act_scale()`` for fp8 storage, the sources' ``_raw_input``.  A slot keeps every variant it was asked
    for: switching dtype or activation domain and back returns the first pack.

What version counters cannot see is covered by ``PackOwner``'s hooks, which drop the owner's whole store: a ``train()`` / ``eval()``
transition (training kernels write parameters and running statistics through raw pointers), ``load_state_dict``, and an ``_apply`` that
moved or cast a tensor (a no-op move keeps the packs).  The hooks see the owner and, through ``nn.Module``'s recursion, the modules
inside it.  What they cannot cover is a slot that reads a module OUTSIDE its owner: ``C2f``'s ``"front"`` reads the stride-2 3x3 in front
of the block, and a raw-pointer write to layers 0 / 1 of the model's ``"stem2"`` goes through those layers' own ``train()``, not the
model's.  Both slots are used only under ``DetectionModel``, whose own ``train()`` / ``eval()`` transition drops every store (``drop_packed``).
"""
from __future__ import annotations

import weakref

import torch

from ... import hip_ops as H

PACKED = "_packed"  # the attribute; ``DetectionModel.drop_packed`` and the checkpoint writer's drop list take it from here


def _tensors(m):
    return list(m.parameters()) + list(m.buffers())


def packed(owner, slot, sources, dtype, device, build, *extras):
    """The pack of ``owner``'s ``slot`` for this variant, from ``build()`` when none is valid.  ``sources``: the modules the fold reads."""
    store = owner.__dict__.setdefault(PACKED, {})
    ent = store.get(slot)
    # (the sources are remembered weakly: the owner is often its own source, and a module in a reference cycle is freed — with everything its
    # parameters' hooks hold, a trainer's hipGraphs among it — by some later garbage collection, possibly inside another graph capture)
    if ent is None or len(ent[0]) != len(sources) or any(r() is not m for r, m in zip(ent[0], sources)):
        ent = store[slot] = [tuple(weakref.ref(m) for m in sources), None, None, {}]
    if ent[1] is None:  # (the module walk costs more than the rest of a hit: the tensor list is kept, as ``weights_signature`` keeps its own)
        ent[1] = [t for m in sources for t in _tensors(m)]
    sig = tuple((t.data_ptr(), t._version) for t in ent[1])
    if ent[2] != sig:
        ent[2], ent[3] = sig, {}
    key = (dtype, torch.device(device), H.scaled_domain(), H.fp8_act_scale() if dtype == H.FP8 else None,
           tuple(getattr(m, "_raw_input", False) for m in sources), *extras)
    pack = ent[3].get(key)
    if pack is None:
        pack = ent[3][key] = build()
    return pack


class PackOwner:
    """Mixin of every module that keeps packs: drops them where torch's version counters do not see the weights change."""

    def invalidate_packed(self) -> None:
        self.__dict__.pop(PACKED, None)

    def train(self, mode: bool = True):
        if mode != self.training:  # a training phase writes the parameters through raw pointers: packs made before it are stale
            self.invalidate_packed()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_packed()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        before = [(t.data_ptr(), t.dtype, t.device) for t in _tensors(self)]
        out = super()._apply(fn, *args, **kwargs)
        if before != [(t.data_ptr(), t.dtype, t.device) for t in _tensors(self)]:
            self.invalidate_packed()  # .to(device) / .half(): a no-op move (second predictor on the same model) keeps the packs
        for ent in self.__dict__.get(PACKED, {}).values():
            ent[1] = None  # (fn may have handed back new tensor objects on the same storage: walk the sources again at the next call)
        return out


class _PackedMixin(PackOwner):
    """A module that is one convolution: ``_pack(dtype, device, cin_pad=None)`` makes its ``H.PackedConv``, slot ``"conv"`` keeps it."""

    def _packed_for(self, x: torch.Tensor) -> H.PackedConv:
        def build():
            pc = self._pack(x.dtype, x.device)
            if pc.groups == 1 and 0 < x.shape[1] - pc.cin < H.chan_gran(x.dtype):
                # zero-padded input channels (image input padded to one 16-byte chunk): pad the taps to match
                pc = self._pack(x.dtype, x.device, cin_pad=x.shape[1])
            return pc

        return packed(self, "conv", (self,), x.dtype, x.device, build, x.shape[1])
