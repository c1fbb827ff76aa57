"""float64 numpy reference of adjoint checkpointing: adjoint_numpy.AdjointModel64 (and obs_numpy.ObsModel64) extended by
checkpoint_adjoint and adjoint_checkpoints as the engine has them.  With the mode on a step writes no tape; before every step of the
window whose index is a multiple of `every` a copy of vc is kept; adjoint_back fills a tape of at most `every` steps again whenever it
is empty, by stepping from the checkpoint of the segment that holds the newest unswept step with the recording on and NO tangent, and
puts the live state back before it returns.  Also an adjoint set (set_adjoints / adjoints, swept over the one tape), and a face of
torch tensors on the CPU over such a model, through which binding.fourdvar and binding.singular_vectors run as they are.  Used ONLY by
tests."""
import copy

import numpy as np

import adjoint_numpy as A
import obs_numpy as O


def slots(steps, every):
    """half spectra of a checkpointed window of `steps` steps apart from the live copy: ceil(steps / every) checkpoints + 4 every"""
    return -(-steps // every) + 4 * every


def checkpoint_every_brute(steps):
    """the K in 1..steps that minimises slots(steps, K), the smallest of equal ones"""
    return min(range(1, steps + 1), key=lambda k: (slots(steps, k), k))


class Checkpointing:
    """the mixin: in front of AdjointModel64 or a class derived from it"""

    every = max_steps = done = left = replayed = 0
    swept = False
    cks = ()
    lcs = None

    def _window_empty(self):
        self.cks, self.done, self.left, self.swept, self.replayed = [], 0, 0, False, 0

    def checkpoint_adjoint(self, every, max_steps=0):
        if every < 0 or (every and max_steps < 1):
            raise ValueError("every < 0 or max_steps < 1")
        super().record_adjoint(0)
        self.every, self.max_steps = int(every), int(max_steps) if every else 0
        self._window_empty()

    def adjoint_checkpoints(self):
        return self.every, self.max_steps, len(self.cks), self.replayed

    def record_adjoint(self, depth):
        super().record_adjoint(depth)
        self.every = self.max_steps = 0
        self._window_empty()

    def adjoint_recorded(self):
        return self.left if self.every else super().adjoint_recorded()

    def set_vort(self, vort):
        super().set_vort(vort)
        self._window_empty()

    def set_spectrum(self, vc):
        super().set_spectrum(vc)
        self._window_empty()

    def step(self, n=1):
        if not self.every:
            return super().step(n)
        if self.swept:
            raise ValueError("the window has been swept: start a new one")
        if self.done + n > self.max_steps:
            raise ValueError("the step would pass max_steps")
        for _ in range(n):
            if self.done % self.every == 0:
                self.cks.append(self.vc.copy())
            super().step(1)                                     # depth == 0: no tape
            self.done += 1
            self.left += 1

    def _refill(self):
        seg = (self.left - 1) // self.every
        count = self.left - seg * self.every
        self.vc, self.dc = self.cks[seg].copy(), None           # the vorticity alone is stepped again
        self.depth = count
        A.AdjointModel64.step(self, count)
        self.depth = 0
        self.replayed += count

    # ---- an adjoint set over the one tape ----
    def set_adjoint(self, lam):
        super().set_adjoint(lam)
        self.lcs = None

    def set_adjoints(self, lams):
        self.lcs = [np.fft.rfft2(np.asarray(a).astype(np.float64)) for a in lams]
        self.lc = self.lcs[0]

    def adjoints(self):
        return np.stack([self._c2r(a) for a in (self.lcs if self.lcs is not None else [self.lc])])

    def _pop(self):
        """the newest step of the tape leaves it, its transpose applied to every variable"""
        if self.lcs is None:
            return super().adjoint_back(1)
        entry = self.tape[-1]
        for i, lam in enumerate(self.lcs):
            if i:
                self.tape.append(entry)
            self.lc = lam
            super().adjoint_back(1)
            self.lcs[i] = self.lc
        self.lc = self.lcs[0]

    def adjoint_back(self, n=1):
        if n < 0 or n > self.adjoint_recorded():
            raise ValueError("more steps than are recorded")
        live = None
        for _ in range(n):
            if self.every and not self.tape:
                if live is None:
                    live = (self.vc, self.dc)
                self._refill()
            self._pop()
            if self.every:
                self.left -= 1
                self.swept = True
        if live is not None:
            self.vc, self.dc = live


class CheckpointModel64(Checkpointing, A.AdjointModel64):
    pass


class CheckpointObs64(Checkpointing, O.ObsModel64):
    pass


class TorchFace:
    """A float64 model behind the methods that binding.fourdvar and binding.singular_vectors call, with torch tensors on the CPU
    (.device tells the helpers where to keep theirs).  A tangent set of k is carried by k - 1 copies of the model that never record."""

    device = "cpu"

    def __init__(self, model):
        import torch
        self.torch, self.m = torch, model
        self._shape = (model.nx, model.ny)
        self.dcs = None

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a))

    def set_vort(self, v): self.m.set_vort(v.numpy())
    def spectrum(self): return self.m.spectrum()
    def set_spectrum(self, z): self.m.set_spectrum(z)
    def record_adjoint(self, depth): self.m.record_adjoint(depth)
    def checkpoint_adjoint(self, every, max_steps=0): self.m.checkpoint_adjoint(every, max_steps)
    def adjoint_back(self, n=1): self.m.adjoint_back(n)
    def set_adjoint(self, lam): self.m.set_adjoint(lam.numpy())
    def adjoint(self): return self._t(self.m.adjoint())
    def set_adjoints(self, lams): self.m.set_adjoints(lams.numpy())
    def adjoints(self): return self._t(self.m.adjoints())
    def observe(self, kind, xy): return self._t(self.m.observe(kind, xy.numpy()))
    def adjoint_add_obs(self, kind, xy, w): self.m.adjoint_add_obs(kind, xy.numpy(), w.numpy())

    def obs_misfit(self, h, y, sigma, cost, check=True):
        d = h - y
        r = d if sigma is None else d / sigma ** 2
        cost += 0.5 * (d * r).sum()
        return r

    def set_tangents(self, v):
        self.dcs = [np.fft.rfft2(a.numpy().astype(np.float64)) for a in v]
        self.m.dc = self.dcs[0]

    def tangents(self):
        return self._t(np.stack([self.m._c2r(a) for a in self.dcs]).astype(np.float32))

    def step(self, n=1):
        if self.dcs is None:
            return self.m.step(n)
        for i in range(1, len(self.dcs)):
            aux = copy.copy(self.m)
            aux.depth, aux.every, aux.tape, aux.dc = 0, 0, [], self.dcs[i]
            A.AdjointModel64.step(aux, n)
            self.dcs[i] = aux.dc
        self.m.dc = self.dcs[0]
        self.m.step(n)
        self.dcs[0] = self.m.dc
