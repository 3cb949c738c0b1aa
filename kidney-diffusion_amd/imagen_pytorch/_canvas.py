"""The driver of one stage of ``Imagen.sample_tiled``: the canvas from x_T to the unnormalised sample, over one shard or
several.  ``_CanvasStage`` is what every shard reads, ``_CanvasShard`` one shard's canvases, tile store and plans on its
device, ``_StripLink`` the strip buffer between two shards.  ``Imagen._tiled_stage`` builds them and runs the slot loop:
per resample slot of the schedule steps skip .. T - 1 every shard denoises its own tiles, the links trade the overlap
strips, every shard takes the canvas step.  One host thread; every call is issued under the shard's device on that
device's current stream, and the shards meet through events alone (nothing waits on the host inside a step)."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _engine as E
from .imagen_pytorch import (_OBJECTIVES, _f32, _stage_noise, _StageIO, _StepSchedule, canvas_tables, cond_crop_maps, exists,
                             log_snr_to_alpha_sigma, resize_image_to)

_int_ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # of an int32 device tensor (E.ptr takes fp32 alone)


class _CanvasStage:
    """What every shard of a stage reads and nobody writes after construction: the geometry ``geo`` (normalize_tiling's) and
    the step tables; ``coefs``, the canvas sampler's coefficients per step (canvas_tables); ``sc``, the tiles' own
    iteration - DDIM(0): first order, no history, no draw, its tile-level update is discarded; ``slots`` [(k, j)] - slot
    j of step k is resample r = R - 1 - j; the low-res ``(ls, a, s)``; ``crops`` = (TileCondCrops, Cs, W, tile channels,
    top, shifts); the known ``(kn, km, R)`` and init ``(init, skip)`` sources - without them R = 1, skip = 0, the sources
    are NULL and a step has one slot; the noise function, the seed and the stage's Philox key."""

    def __init__(self, imagen, unet, stage, geo, sched, objective, dynamic_threshold, prev_canvas, cond_images, lowres_level,
                 noise_fn, seed, use_graph, tile_batch, text_embeds, text_masks, cond_scale, solver, streamed, crops, known, start):
        self.lib, self.imagen, self.unet, self.stage, self.geo, self.objective = E.load(), imagen, unet, stage, geo, objective
        self.dynamic_threshold, self.prev_canvas, self.cond_images, self.noise_fn = dynamic_threshold, prev_canvas, cond_images, noise_fn
        self.seed, self.use_graph, self.tile_batch, self.streamed, self.crops = seed, use_graph, tile_batch, streamed, crops
        self.text = (text_embeds, text_masks, cond_scale) if exists(text_embeds) and unet.cond_on_text else None
        (self.kn, self.km, self.R), (self.init, self.skip) = known, start
        self.shape = (1, imagen.channels, geo["Hc"], geo["Wc"])
        self.key = _stage_noise(self.lib, noise_fn, seed, stage, None)[1]
        self.tables = sched.step_tables()
        self.coefs = canvas_tables(self.tables, *solver, skip=self.skip)
        self.third = "coef_prev2" in self.coefs and bool(self.coefs["coef_prev2"].any())   # some step reads the estimate of step k - 2
        self.multistep = bool(self.coefs["coef_prev"].any())                               # some step reads the estimate of step k - 1
        self.sc = _StepSchedule(self.tables, "ddim", eta=0.0)
        self.T, self.tile_steps = self.sc.T, getattr(self.lib, self.sc.steps)
        self.slots = [(k, j) for k in range(self.skip, self.T) for j in range(self.R)]
        self.ls = self.a = self.s = None
        if unet.lowres_cond:
            self.ls = imagen.lowres_noise_schedule.log_snr(torch.full((1,), lowres_level, dtype=torch.float32))
            self.a, self.s = (float(v) for v in log_snr_to_alpha_sigma(self.ls))
        Ct = crops[3] if exists(crops) else cond_images.shape[1] if exists(cond_images) else unet.cond_images_channels
        assert Ct == unet.cond_images_channels, "invalid number of channels in conditioning image"

    def covered(self):
        """The torch finish's host mask of the pixels a tile covers: built once per stage, for all shards, and at the end -
        behind the launches of the last slot, so that the host builds it while the devices work."""
        covered = torch.zeros(self.shape[2:], dtype=torch.bool)
        for ty, tx in self.geo["origins"]:
            covered[ty:ty + self.geo["S"], tx:tx + self.geo["S"]] = True
        return covered

    def mix(self, k):
        """(a, s) of the mix of the known pixels before a slot of step k."""
        return float(self.tables["alpha"][k]), float(self.tables["sigma"][k])


class _CanvasShard:
    """One shard of a stage on ``dev``: ``lay`` is its dict of normalize_shards.  It holds the WHOLE canvas - ``x``, the
    fused estimate, under 3M the one before it, under 2M / 3M with resampling the slot's estimate - and a tile store of
    its own and halo tiles, with a ``tile_of`` for exactly that set; it starts the canvas itself (the bits are a function
    of the canvas element) and denoises its OWN tiles with plans of its own (``replica`` = its number).

    THE INVARIANT: after the canvas step every pixel of the shard's band extent - the canvas rows its own tiles cover -
    holds the bits of the single-shard canvas, in x, in the fused estimate, in the history and so in the
    self-conditioning carry gathered from it.  Every tile covering such a pixel is an own or a halo tile and covers it
    inside its strip, the fusion order follows the lattice slot and not the store, the update is pointwise and its noise
    is keyed by the canvas element; so the next gather of the own tiles, which reads nothing outside the extent, reads
    only exact pixels.  Outside its extent a shard's canvas holds garbage (fused from halo rows that were never sent) and
    is never read.

    The previous canvas, the conditioning source, the known image, the mask and the init image are copied to the device
    once per stage; a source already there is read in place - a view of the caller's tensor, described to the kernels.
    Every method runs under ``torch.cuda.device(dev)``, which the caller sets."""

    def __init__(self, stage, num, dev, lay):
        st = self.st = stage
        unet, (_, Cn, Hc, Wc), S = st.unet, st.shape, st.geo["S"]
        f32 = lambda t: _f32(t, dev)
        new = lambda fill=torch.empty, shape=st.shape: fill(shape, device=dev, dtype=torch.float32)
        self.num, self.dev, self.tiles, self.N, self.owned = num, dev, lay["tiles"], len(lay["tiles"]), lay["owned"]
        self.halo = [self.tiles.index(t) for t in lay["halo"]]   # the store slots of the halo tiles
        here = lambda t: t.is_cuda and t.device.index == (torch.cuda.current_device() if dev.index is None else dev.index)
        self.kn, self.init = (t if t is None or here(t) else f32(t) for t in (st.kn, st.init))
        self.km = st.km if st.km is None or here(st.km) else st.km.to(dev)
        self.kn_s, self.km_s, self.init_s = E.tiles_image(self.kn), E.tiles_mask(self.km), E.tiles_image(self.init)
        self.x = new()
        # why x0bar_slot exists - a multistep solver under resampling: the history takes a step's estimate in its last slot
        # only, the slots before it leave theirs (a self-conditioned UNet's carry) in a canvas of their own (written before
        # it is read)
        self.x0bar_slot = new() if st.R > 1 and st.multistep else None
        # third order: a ring of three canvases - x0bar, x0bar2 and the one being written, which is x0bar2 again: the
        # estimate of step k overwrites that of step k - 2, each thread behind its own read, and two pointers swap
        self.x0bar, self.x0bar2 = new(torch.zeros), new(torch.zeros) if st.third else None
        self.latest = self.x0bar   # the canvas that holds the fused estimate of the previous slot
        self.store = new(shape=(self.N, Cn, S, S))
        self.thr = new(shape=(self.N,)) if st.dynamic_threshold else None
        self.tile_of = torch.tensor(lay["tile_of"], dtype=torch.int32).to(dev).contiguous()
        self.lowres = self.lowres_z = self.prev = self.cond = self.src = None
        if unet.lowres_cond and st.streamed:   # no canvas is built: every chunk is cut out of prev_canvas (injected noise stays a canvas)
            self.prev = f32(st.prev_canvas)
            assert self.prev.dim() == 4 and tuple(self.prev.shape[:2]) == (1, Cn), "the previous canvas must be [1, C, H, W]"
            self.lowres_z = f32(st.noise_fn(("lowres", st.stage), st.shape)) if exists(st.noise_fn) else None
        elif unet.lowres_cond:   # the previous canvas resized to this one and augmented ONCE: overlapping tiles share it
            gauss = _stage_noise(st.lib, st.noise_fn, st.seed, st.stage, dev)[0]
            lowres = F.interpolate(st.prev_canvas.to(dev), (Hc, Wc), mode="nearest") * 2 - 1
            self.lowres = (st.a * lowres + st.s * gauss(("lowres", st.stage), st.shape, (16 << 32) | 1)).contiguous()
        if exists(st.cond_images):
            self.cond = f32(resize_image_to(f32(st.cond_images), S))
        elif exists(st.crops):
            cc = st.crops[0]
            self.src = f32(cc.image.float() / 255.0 if cc.image.dtype == torch.uint8 else cc.image)   # moved once; stays for the stage
            self.win_of, self.centre_of = (None if m is None else m.to(dev) for m in cond_crop_maps(cc.window, S, cc.centre_width))
        cond_shape = tuple(self.cond.shape[1:]) if exists(self.cond) else (st.crops[3], S, S) if exists(st.crops) else None
        # one plan, one set of stable buffers and one argument struct per batch size (the full chunks' and the ragged one's)
        own, tb, plans = lay["own"], st.tile_batch, {}
        for b in sorted({min(tb, len(own) - n0) for n0 in range(0, len(own), tb)}):
            io = _StageIO(st.imagen, unet, b, S, dev, dynamic_threshold=st.dynamic_threshold, use_graph=st.use_graph, key=st.key,
                          replica=num)   # (DDIM(0) draws nothing)
            io.args.objective = _OBJECTIVES[st.objective]
            p = plans[b] = dict(io=io, args=io.args, img=io.buf("img", (b, Cn, S, S)))
            if unet.lowres_cond:
                p["lowres"] = io.buf("lowres", (b, Cn, S, S))
                io.args.d_lowres = E.ptr(p["lowres"])
                io.lowres_level(st.ls)
            if exists(cond_shape):
                p["cond"] = io.buf("cond", (b,) + cond_shape)
                io.args.d_cond_images = E.ptr(p["cond"])
            if unet.self_cond:
                p["self_cond"] = io.buf("tile_self_cond", (b, Cn, S, S))
            p["h"] = unet.engine(b, S, dev, with_text=exists(st.text), replica=num)
            if exists(st.text):   # one row for the canvas, given to every tile of the chunk
                rows = lambda t: None if t is None else t.expand(b, *t.shape[1:])
                io.text(p["h"], rows(st.text[0]), rows(st.text[1]), st.text[2])
        # per chunk of at most tile_batch own tiles: its first tile on the canvas, its slot in the store, its batch, its plan
        # and the ctypes arrays of its tiles' origins and conditioning shifts
        flat = lambda pairs: (C.c_int * (2 * len(pairs)))(*[v for p in pairs for v in p])
        self.chunks = [(t0, lay["base"] + t0 - own[0], b, plans[b], flat(st.geo["origins"][t0:t0 + b]),
                        flat(st.crops[5][t0:t0 + b]) if exists(st.crops) else None)
                       for t0 in range(own[0], own[0] + len(own), tb) for b in (min(tb, own[0] + len(own) - t0),)]

    def inject(self, kind, k, j):
        """The injected draw of a kind for slot j of step k, on the device; None where Philox draws.  The tensor is memory
        of torch's current stream: the allocator hands it on only behind the launch that reads it."""
        st = self.st
        return _f32(st.noise_fn((kind, st.stage, k, st.R - 1 - j), st.shape), self.dev) if exists(st.noise_fn) else None

    def start(self):
        """x_T, plus the init image, with the first mix of the known pixels (kd_tiles_start).  Scale 1, no image, no mask:
        1.0 * z, the bits of the draw itself."""
        st = self.st
        z, zm = (_f32(st.noise_fn(("init", st.stage), st.shape), self.dev) if exists(st.noise_fn) else None,
                 self.inject("inpaint", st.skip, 0) if exists(st.kn) else None)
        E.check(st.lib.kd_tiles_start(E.ptr(self.x), *st.shape[1:], st.imagen._start_scale(st.stage), E.ptr(z), st.key,
                                      E.ref(self.init_s), E.ref(self.kn_s), E.ref(self.km_s), *st.mix(st.skip), E.ptr(zm),
                                      E.stream_id(2, st.skip * st.R), E.current_stream()))

    def poison_halo(self):
        """For tests alone: NaN in every halo slot of the store, and in its threshold, so that only the received strips hold
        numbers."""
        for t in filter(exists, (self.store, self.thr) if self.halo else ()):
            t[self.halo] = float("nan")

    def denoise(self, i, k):
        """The own tiles through slot i (of step k), chunk by chunk: gathered out of the canvas into the plan's stable
        buffers, one iteration of the tiles' schedule, the x0 estimates and thresholds into the store.  A ragged last chunk
        runs the plan of its own batch size."""
        st, lib, unet, stream, (_, Cn, Hc, Wc), S = self.st, self.st.lib, self.st.unet, E.current_stream, self.st.shape, self.st.geo["S"]
        gather = lambda src, dst, b, yx: E.check(lib.kd_tiles_gather(E.ptr(src), E.ptr(dst), b, Cn, Hc, Wc, S, yx, stream()))
        for t0, at, b, p, yx, shifts in self.chunks:
            gather(self.x, p["img"], b, yx)
            if exists(self.prev):   # a (2 nearest(prev_canvas) - 1) + s z over the chunk's tiles
                E.check(lib.kd_tiles_gather_lowres(E.ptr(self.prev), *self.prev.shape[2:], E.ptr(p["lowres"]), b, Cn, Hc, Wc, S, yx,
                                                   st.a, st.s, E.ptr(self.lowres_z), st.key, (16 << 32) | 1, stream()))
            elif exists(self.lowres):
                gather(self.lowres, p["lowres"], b, yx)
            if exists(self.cond):
                p["cond"].copy_(self.cond[t0:t0 + b])
            elif exists(self.src):   # the conditioning windows of the chunk's tiles, cut out of the one image
                cc, Cs, W, _, top, _ = st.crops
                E.check(lib.kd_tiles_cond_gather(E.ptr(self.src), Cs, W, E.ptr(p["cond"]), b, S, shifts, top, _int_ptr(self.win_of),
                                                 _int_ptr(self.centre_of), float(cc.fill), stream()))
            if unet.self_cond and i > 0:   # the carry is the FUSED estimate of the slot before (the first starts from zeros)
                gather(self.latest, p["self_cond"], b, yx)
                E.check(lib.kd_sample_set_self_cond(p["h"], E.ptr(p["self_cond"]), stream()))
            elif unet.self_cond and k > 0:   # a first step walked behind step 0: the plan holds another call's carry
                E.check(lib.kd_sample_set_self_cond(p["h"], None, stream()))
            p["args"].keep_self_cond = int(i > 0)   # (the later slots of step 0 keep the carry just set)
            E.check(st.tile_steps(p["h"], C.byref(st.sc.struct), C.byref(p["args"]), E.ptr(p["img"]), k, k + 1, stream()))
            E.check(lib.kd_sample_last(p["h"], 1, E.ptr(self.store[at:at + b]), stream()))
            if exists(self.thr):
                E.check(lib.kd_sample_last(p["h"], 2, E.ptr(self.thr[at:at + b]), stream()))

    def step(self, i, k, j):
        """The canvas step of slot i = (k, j) over own and halo tiles: ONE kd_tiles_fuse_update_hist2 with the canvas
        sampler's coefficients of step k - fusion, update, re-noise and the next slot's mix in the one canvas pass."""
        st, geo = self.st, self.st.geo
        # (a sampler without a second history: no coef_prev2, or zeros all through - P2 = 0 and x0bar2 is NULL)
        A, B, P, Sn, P2 = (float(st.coefs[c][k]) if c in st.coefs else 0.0
                           for c in ("coef_x", "coef_x0", "coef_prev", "coef_noise", "coef_prev2"))
        it, renoise = k * st.R + j, j < st.R - 1 and k < st.T - 1
        nxt = st.slots[i + 1] if exists(st.kn) and i + 1 < len(st.slots) else None   # the last slot mixes nothing: the end pastes
        # the draws stay in locals over the launch: a tensor released before it would be handed to the next allocation
        z, zr = self.inject("step", k, j) if Sn != 0.0 else None, self.inject("renoise", k, j) if renoise else None
        zm = self.inject("inpaint", *nxt) if exists(nxt) else None
        last = j == st.R - 1 or self.x0bar_slot is None
        est = (self.x0bar2 if st.third else self.x0bar) if last else self.x0bar_slot
        E.check(st.lib.kd_tiles_fuse_update_hist2(
            E.ptr(self.x), E.ptr(self.x0bar), E.ptr(est), E.ptr(self.store), E.ptr(self.thr), _int_ptr(self.tile_of), self.N, st.shape[1],
            geo["S"], geo["st"], geo["ny"], geo["nx"], int(geo["weights"] == "ramp"), A, B, P, Sn,
            E.ptr(z), st.key, E.stream_id(1, it), int(renoise), float(st.tables["rn_a"][k]), float(st.tables["rn_b"][k]), E.ptr(zr),
            E.stream_id(3, it),
            *((E.ref(self.kn_s), E.ref(self.km_s), *st.mix(nxt[0]), E.ptr(zm), E.stream_id(2, nxt[0] * st.R + nxt[1]))
              if exists(nxt) else (None, None, 0.0, 0.0, None, 0)),
            E.ptr(self.x0bar2), P2, E.current_stream()))
        if st.third and last:   # the ring advances: this step's estimate is the next step's first history
            self.x0bar, self.x0bar2 = self.x0bar2, self.x0bar
        self.latest = est

    def finish_rows(self, out, oy, ox, is_head):
        """The end of a streamed stage over the canvas rows this shard owns, one pass (kd_tiles_finalize_rows): the covered
        pixels clamped into the window of ``out`` at (oy, ox), the known pixels pasted, nothing else touched.  The head
        shard writes straight into ``out``, on its device; another into a band of its rows that one copy takes there."""
        st, geo, (y0, y1), Wc = self.st, self.st.geo, self.owned, self.st.shape[3]
        band, by, bx = out, oy, ox
        if not is_head:
            window = out[:, :, oy + y0:oy + y1, ox:ox + Wc]
            band, by, bx = torch.empty((1, st.shape[1], y1 - y0, Wc), device=self.dev, dtype=torch.float32), -y0, 0
            if len(geo["origins"]) < geo["ny"] * geo["nx"]:   # an uncovered pixel keeps the destination's bits: the band starts from them
                band.copy_(window, non_blocking=True)
        E.check(st.lib.kd_tiles_finalize_rows(E.ptr(self.x), _int_ptr(self.tile_of), self.N, st.shape[1], geo["S"], geo["st"], geo["ny"],
                                              geo["nx"], E.ptr(band), *band.shape[2:], by, bx, E.ref(self.kn_s), E.ref(self.km_s),
                                              y0, y1, E.current_stream()))
        if not is_head:
            with torch.cuda.device(out.device):
                window.copy_(band, non_blocking=True)

    def finish_torch(self, covered):
        """The same clamp and paste in torch, over the rows this shard owns (``covered``: _CanvasStage.covered()): the
        reference the tests hold the kernel to."""
        st, (y0, y1) = self.st, self.owned
        out = (self.x[:, :, y0:y1].clamp(-1.0, 1.0) + 1) * 0.5
        if exists(self.kn):   # the paste on nearest-resized copies
            resized = lambda t: t if t.shape[-2:] == st.shape[2:] else F.interpolate(t, st.shape[2:], mode="nearest")
            out = torch.where(resized(self.km[None, None].float())[:, :, y0:y1] != 0, resized(self.kn)[:, :, y0:y1], out)
        return torch.where(covered[y0:y1].to(self.dev), out, torch.zeros_like(out))


class _StripLink:
    """One pair of shards with strips to send: ``items`` = [(tile, row0, rows)] of normalize_shards' ``exchange``.  The strips
    of ``src``'s boundary tiles' estimates travel with their thresholds - kd_tiles_rows_copy packs them into one buffer
    ``[n strips of C x rows x S | n thresholds]`` (one allocation: what travels is one contiguous buffer), one ``copy_`` moves
    it, kd_tiles_rows_copy unpacks it into ``dst``'s halo slots.

    The event discipline of the strip buffer: ``ready`` is recorded behind the pack and the copy waits for it; ``freed`` is
    recorded behind the copy, and the next pack waits for it - the buffer is written again only behind the copy that read
    it."""

    def __init__(self, stage, src, dst, items):
        self.st, self.src, self.dst, self.n, self.rows = stage, src, dst, len(items), max(r for _, _, r in items)
        self.ready, self.freed, self.sent = torch.cuda.Event(), torch.cuda.Event(), False
        flat = lambda quads: (C.c_int * (4 * self.n))(*[v for q in quads for v in q])
        self.pack = flat((src.tiles.index(t), m, r0, r) for m, (t, r0, r) in enumerate(items))
        self.unpack = flat((m, dst.tiles.index(t), r0, r) for m, (t, r0, r) in enumerate(items))
        self.words = self.n * stage.shape[1] * self.rows * stage.geo["S"]
        self.out = torch.empty(self.words + self.n, device=src.dev, dtype=torch.float32)
        self.inn = torch.empty(self.words + self.n, device=dst.dev, dtype=torch.float32)

    def trade(self):
        """The strips of the pair: packed where they were made, moved, unpacked into the halo slots."""
        st, src, dst, n, rows, Cn, S = self.st, self.src, self.dst, self.n, self.rows, self.st.shape[1], self.st.geo["S"]
        tail = lambda buf: C.c_void_p(buf.data_ptr() + 4 * self.words) if st.dynamic_threshold else None
        with torch.cuda.device(src.dev):
            if self.sent:
                torch.cuda.current_stream().wait_event(self.freed)
            E.check(st.lib.kd_tiles_rows_copy(E.ptr(src.store), src.N, S, E.ptr(self.out), n, rows, E.ptr(src.thr), tail(self.out),
                                              n, Cn, S, self.pack, E.current_stream()))
            self.ready.record()
        with torch.cuda.device(dst.dev):
            torch.cuda.current_stream().wait_event(self.ready)
            self.inn.copy_(self.out, non_blocking=True)
            self.freed.record()
            self.sent = True
            E.check(st.lib.kd_tiles_rows_copy(E.ptr(self.inn), n, rows, E.ptr(dst.store), dst.N, S, tail(self.inn), E.ptr(dst.thr),
                                              n, Cn, S, self.unpack, E.current_stream()))
