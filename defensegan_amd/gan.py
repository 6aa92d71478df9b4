"""Host-side mirror of the reference's GAN model object for the latent-projection path.

Keeps the surface of ``DefenseGANBase`` (/root/reference/models/gan.py:39-647) that the callers of
the hot path use -- ``GAN(cfg, test_mode=True)``, ``.load_generator()``, ``.reconstruct(images,
batch_size, back_prop, reconstructor_id, z_init_val)``, attributes ``rec_iters / rec_rr / rec_lr /
latent_dim / net_dim / use_bn / image_dim / batch_size / dataset_name`` -- and forwards the work to
the hand-written HIP engine through the C ABI (include/defensegan_hip.h).  Arrays replace TF tensors:
NumPy in -> NumPy out, torch in -> torch (on the engine's device) out.

Differences from the reference that are deliberate:
* stateless per call: fresh z0 / zero momentum every batch (what ``model_eval_gan`` arranges with
  ``tf.local_variables_initializer()``, utils/gan_defense.py:119); no warm start across batches;
* ragged last batches are accepted (the reference's static graph needs exactly ``batch_size`` images);
* the learning rate is the constant ``rec_lr`` -- what the reference executes, because the decay's
  step variable is never advanced (gan.py:362-386, base_model.py:188-192).
There is no CPU fallback: without the HIP library / a GPU every compute method raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import _native, archs, config as _config


def _torch():
    import torch
    return torch


class DefenseGANBase(object):
    arch_name = None          # set by subclasses

    _default_attributes = ['dataset_name', 'batch_size', 'use_bn', 'test_batch_size', 'latent_dim',
                           'net_dim', 'rec_iters', 'image_dim', 'rec_rr', 'rec_lr', 'debug',
                           'mode', 'gradient_penalty_lambda', 'critic_iters', 'train_iters']

    def __init__(self, cfg=None, test_mode=False, verbose=False, device=None, measure=False, **args):
        # defaults of DefenseGANBase.__init__ (gan.py:50-68)
        self.dataset_name = None
        self.batch_size = 32
        self.use_bn = True
        self.test_batch_size = 20
        self.latent_dim = None
        self.net_dim = None
        self.debug = False
        self.rec_iters = 200
        self.image_dim = [None, None, None]
        self.rec_rr = 10
        self.rec_lr = 10.0
        self.rec_momentum = 0.7            # hard-coded in the reference (gan.py:390)
        # training (gan.py:54-57).  MODE is 'wgan-gp' in every shipped configuration of the reference (experiments/cfgs/gans/);
        # the class default there, 'gp-wgan', matches no branch of _loss
        self.mode = 'wgan-gp'
        self.gradient_penalty_lambda = 10.0
        self.critic_iters = 5
        self.train_iters = 30000
        self.penalty_axes = args.get("penalty_axes", "reference")      # critic.PENALTY_AXES: the reference's height-only sum
        self._critic = None
        # "constant": lr == rec_lr throughout = what the reference executes (its decay never fires, gan.py:362-386);
        # "intended": the x0.1 staircase at ceil(0.8 * rec_iters) its code asks for.  Off by default.
        self.rec_lr_schedule = args.get("rec_lr_schedule", "constant")
        self.test_mode = test_mode
        self.verbose = verbose
        self.cfg = dict(cfg) if cfg else {}
        self.initialized = False
        # attribute resolution order of AbstractModel._set_attr (base_model.py:120-148):
        # explicit keyword > cfg[UPPER] > cfg[lower] > class default
        for name in self._default_attributes:
            val = args.get(name)
            if val is None:
                if name.upper() in self.cfg:
                    val = self.cfg[name.upper()]
                elif name.lower() in self.cfg:
                    val = self.cfg[name.lower()]
            if val is not None:
                setattr(self, name, val)
        if self.latent_dim is None:
            self.latent_dim = 128
        if self.net_dim is None:
            self.net_dim = 64
        self._arch = archs.make_arch(self.arch_name or self.dataset_name, int(self.latent_dim), int(self.net_dim))
        if self.image_dim is None or self.image_dim[0] is None:
            self.image_dim = list(self._arch.image_dim)
        if list(self.image_dim) != list(self._arch.image_dim):
            raise ValueError("image_dim %r does not match the %s generator (%r)" %
                             (self.image_dim, self._arch.name, self._arch.image_dim))
        if test_mode:
            self.test_batch_size = self.batch_size        # gan.py:105
        self._device = device
        self._measure = bool(measure)       # True: the -DDG_MEASURE build of the library (tools/, cross-check tests)
        self._handle = None
        self._weights: Dict[str, np.ndarray] = {}
        self._default_seed = 11241990                     # whitebox.py:143 / blackbox.py:464
        self._calls = 0

    # ------------------------------------------------------------------ engine plumbing
    def _lib(self):
        return _native.load(self._measure)

    def _check(self, rc):
        _native.check(rc, self._lib())

    def _ensure_handle(self):
        if self._handle is not None:
            return self._handle
        torch = _torch()
        lib = self._lib()
        if not torch.cuda.is_available():
            raise _native.NativeError("no GPU visible: the projection engine has no CPU fallback")
        dev = self._device
        if dev is None:
            dev = torch.cuda.current_device()
        if isinstance(dev, str):
            dev = torch.device(dev)
        if hasattr(dev, "index"):
            dev = dev.index if dev.index is not None else torch.cuda.current_device()
        self._device = int(dev)
        h = C.c_void_p()
        self._check(lib.dg_create(self._arch.arch_id, int(self.latent_dim), int(self.net_dim),
                                    1 if self.use_bn else 0, self._device, C.byref(h)))
        self._handle = h
        for k, v in self._weights.items():
            self._push_weight(k, v)
        self._lr_schedule_set = "constant"
        return h

    def _push_weight(self, name: str, arr: np.ndarray):
        lib = self._lib()
        a = np.ascontiguousarray(arr, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        self._check(lib.dg_set_weights(self._handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape,
                                         a.ndim, 0))

    def close(self):
        if self._handle is not None:
            self._lib().dg_destroy(self._handle)
            self._handle = None
        if getattr(self, "_critic", None) is not None:
            self._critic.close()
            self._critic = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def set_weights(self, weights: Dict[str, np.ndarray]):
        """weights: tflib parameter name -> array in the reference layout
        (tflib/__init__.py:9-33; names listed in include/defensegan_hip.h)."""
        want = archs.weight_shapes(self._arch, bool(self.use_bn))
        for k, v in weights.items():
            if k not in want:
                continue
            v = np.asarray(v)
            if k.endswith(".scale") or k.endswith(".offset"):
                # tflib Batchnorm stores these with the keep_dims shape of the moments: [1,4096] for BN1,
                # [1,1,1,C] for BN2/BN3 (tflib/ops/batchnorm.py:83-89); any shape with C values is accepted
                if v.size != int(np.prod(want[k])):
                    raise ValueError("%s: shape %r, expected %d values" % (k, tuple(v.shape), int(np.prod(want[k]))))
                v = v.reshape(want[k])
            elif tuple(v.shape) != tuple(want[k]):
                raise ValueError("%s: shape %r, expected %r" % (k, tuple(v.shape), want[k]))
            self._weights[k] = np.ascontiguousarray(v, np.float32)
            if self._handle is not None:
                self._push_weight(k, self._weights[k])
        missing = [k for k in want if k not in self._weights]
        self.initialized = not missing
        return missing

    def load_generator(self, ckpt_path: Optional[str] = None):
        """Counterpart of ``load_generator`` (gan.py:85-87 -> base_model.py:294-335).  ``ckpt_path`` is

        * an ``.npz`` weight pack whose keys are the tflib parameter names (or a directory holding ``generator.npz``), or
        * a TensorFlow checkpoint written by the reference: a directory with a ``checkpoint`` state file (resolved like
          ``tf.train.get_checkpoint_state``), a checkpoint prefix, or its ``.index`` file -- read without TensorFlow by
          ``tf_checkpoint`` (V2 tensor-bundle format; variables are matched by the last component of their name, so
          ``Generator.Input/Generator.Input.W`` and optimizer slots in the same file are handled).
        """
        if ckpt_path is None:
            ckpt_path = getattr(self, "checkpoint_dir", None)
        if ckpt_path is None:
            raise ValueError("load_generator needs the path of an .npz weight pack or of a TensorFlow checkpoint")
        if os.path.isdir(ckpt_path) and os.path.exists(os.path.join(ckpt_path, "generator.npz")):
            ckpt_path = os.path.join(ckpt_path, "generator.npz")
        if ckpt_path.endswith(".npz"):
            with np.load(ckpt_path) as f:
                weights = {k: f[k] for k in f.files}
        else:
            from . import tf_checkpoint
            expected = archs.weight_shapes(self._arch, bool(self.use_bn))
            weights = tf_checkpoint.generator_weights(ckpt_path, expected.keys())
        missing = self.set_weights(weights)
        if missing:
            raise ValueError("%s lacks %s" % (ckpt_path, ", ".join(missing)))
        return True

    def save_ds(self, splits, root: str = "data/cache", test_again: bool = False):
        """Counterpart of ``save_ds`` (gan.py:604-646): ``<root>/<dataset>_pkl/<split>/feats.pkl`` holding two consecutive
        pickles, the transformed images ``[n,H,W,C]`` (``input_transform`` of the raw [0,255] data) and the targets.
        ``splits``: {'train'|'dev'|'test': (raw images, targets)}.  Written by ``py2pickle`` (protocol 2, Python-2-era
        NumPy module paths) so the Python-2 reference can read it."""
        from . import py2pickle
        out = {}
        for split, (images, targets) in splits.items():
            out_dir = os.path.join(root, "{}_pkl".format(self.dataset_name or self.arch_name), split)
            os.makedirs(out_dir, exist_ok=True)
            path = os.path.join(out_dir, "feats.pkl")
            out[split] = path
            if os.path.exists(path) and not test_again:
                continue
            x = self.input_transform(np.asarray(images, np.float32)).reshape([-1] + list(self.image_dim)).astype(np.float32)
            with open(path, "wb") as f:
                py2pickle.dump(x, f)
                py2pickle.dump(np.asarray(targets), f)
        return out

    # ------------------------------------------------------------------ the hot path
    def input_transform(self, X):
        """[0,255] -> generator range: /255 for MNIST / F-MNIST (gan.py:684-685, 697-698),
        2*(x/255 - .5) for CelebA (gan.py:764-765)."""
        if self._arch.arch_id == archs.ARCH_CELEBA:
            return 2.0 * (X / 255.0 - 0.5)
        return X / 255.0

    def _to_device(self, a, dtype=None):
        torch = _torch()
        dev = torch.device("cuda", self._device)
        if isinstance(a, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(a))
        else:
            t = a
        t = t.to(device=dev, dtype=dtype or torch.float32)
        return t.contiguous()

    def reconstruct(self, images, batch_size=None, back_prop=True, reconstructor_id=0, z_init_val=None,
                    seed=None, first_row=0, return_details=False):
        """Defense-GAN projection of ``images`` [B,H,W,C] (already in generator range).

        Same arguments as the reference (gan.py:333-335).  ``batch_size`` only validates the leading
        dimension when given (the reference needs it for its static graph); ``back_prop`` is accepted and
        ignored -- the reference's gradient through this op is identically zero;
        ``reconstructor_id`` only named TF variables.  ``z_init_val`` [B*rec_rr, latent] fixes z0
        (row b*rec_rr + r, gan.py:348-359, 395-397); otherwise rows are drawn N(0, 1/latent) on the
        device from (seed, first_row + row).  Returns the reconstructions [B,H,W,C]; with
        ``return_details`` a dict with rec, idx [B], loss [B*R], z [B*R, latent].
        """
        self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        torch = _torch()
        lib = self._lib()
        was_numpy = isinstance(images, np.ndarray)
        x = self._to_device(images)
        H, W, Cc = self._arch.image_dim
        if x.dim() == 2 and x.shape[1] == H * W * Cc:
            x = x.view(-1, H, W, Cc)
        if x.dim() != 4 or tuple(x.shape[1:]) != (H, W, Cc):
            raise ValueError("images must be [B,%d,%d,%d], got %r" % (H, W, Cc, tuple(x.shape)))
        B = int(x.shape[0])
        if batch_size is not None and B > int(batch_size):
            raise ValueError("got %d images for batch_size=%d" % (B, batch_size))
        R, L = int(self.rec_rr), int(self.rec_iters)
        n_rows = B * R
        if self.rec_lr_schedule != self._lr_schedule_set:
            self._check(lib.dg_set_option(self._handle, b"lr_schedule", str(self.rec_lr_schedule).encode()))
            self._lr_schedule_set = self.rec_lr_schedule
        z0 = None
        if z_init_val is not None:
            z0 = self._to_device(z_init_val)
            if tuple(z0.shape) != (n_rows, int(self.latent_dim)):
                raise ValueError("z_init_val must be [%d,%d], got %r" % (n_rows, self.latent_dim, tuple(z0.shape)))
        if seed is None:
            seed = self._default_seed + self._calls
        self._calls += 1
        dev = x.device
        rec = torch.empty_like(x)
        idx = torch.empty(B, dtype=torch.int32, device=dev)
        loss = torch.empty(n_rows, dtype=torch.float32, device=dev)
        zout = torch.empty(n_rows, int(self.latent_dim), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            self._check(lib.dg_reconstruct(
                self._handle, x.data_ptr(), z0.data_ptr() if z0 is not None else None,
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_row), B, R, L, float(self.rec_lr), float(self.rec_momentum),
                rec.data_ptr(), idx.data_ptr(), loss.data_ptr(), zout.data_ptr(), stream))
        if return_details:
            out = {"rec": rec, "idx": idx, "loss": loss, "z": zout}
            if was_numpy:
                out = {k: v.cpu().numpy() for k, v in out.items()}
            return out
        return rec.cpu().numpy() if was_numpy else rec

    def row_groups(self, batch_size=None) -> int:
        """Number of row groups a ``reconstruct`` of ``batch_size`` images runs as (dg_call_row_groups; option ``two_streams``)."""
        h = self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        lib = self._lib()
        n = lib.dg_call_row_groups(h, int(batch_size or self.test_batch_size), int(self.rec_rr))
        if n < 0:
            raise _native.NativeError(lib.dg_last_error().decode())
        return int(n)

    def prepare(self, batch_size=None):
        """Builds everything ``reconstruct`` needs for batches of ``batch_size`` images (workspace, the per-layer job lists
        chosen by timing) ahead of the first call -- the counterpart of the reference building its static graph for
        ``batch_size * rec_rr`` rows (gan.py:345-377).  Optional: an unprepared ``reconstruct`` prepares itself, blocking
        once per new batch size; after ``prepare`` the call only enqueues work on the stream (dg_prepare)."""
        self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        torch = _torch()
        dev = torch.device("cuda", self._device)
        B = int(batch_size or self.test_batch_size)
        # DG_TUNING_CACHE=<file>: job-list choices made by an earlier process (the bench, before a profiler pass) are installed
        # instead of being timed again, and this process's own choices are written back -- both runs then launch the same lists
        cache = os.environ.get("DG_TUNING_CACHE")
        if cache and os.path.exists(cache) and not getattr(self, "_tuning_cache_loaded", False):
            self._tuning_cache_loaded = True
            try:
                with open(cache) as fh:
                    self.import_tuning(fh.read())
            except (_native.NativeError, OSError) as e:          # another configuration / device: tune afresh
                if self.verbose:
                    print("[defensegan_amd] %s ignored: %s" % (cache, e))
        with torch.cuda.device(dev):
            self._check(self._lib().dg_prepare(self._handle, B, int(self.rec_rr),
                                                    torch.cuda.current_stream(dev).cuda_stream))
        if cache:
            text = self.export_tuning()
            try:
                old = open(cache).read() if os.path.exists(cache) else None
                if old != text:
                    tmp = "%s.%d.tmp" % (cache, os.getpid())
                    with open(tmp, "w") as fh:
                        fh.write(text)
                    os.replace(tmp, cache)
            except OSError:
                pass

    # ------------------------------------------------------------------ tuning hand-over (dg_export_tuning / dg_import_tuning)
    def export_tuning(self) -> str:
        """The job-list choices of this handle as text (one line per GEMM layer and row count)."""
        self._ensure_handle()
        lib = self._lib()
        need = int(lib.dg_export_tuning(self._handle, None, 0))
        if need < 0:
            self._check(need)
        buf = C.create_string_buffer(need)
        got = int(lib.dg_export_tuning(self._handle, C.cast(buf, C.c_void_p), need))
        if got < 0:
            self._check(got)
        return buf.value.decode()

    def import_tuning(self, text: str) -> int:
        """Installs the choices of another handle's ``export_tuning`` (same architecture, options and CU count) without timing;
        returns the number of lists installed."""
        self._ensure_handle()
        n = int(self._lib().dg_import_tuning(self._handle, text.encode()))
        if n < 0:
            self._check(n)
        return n

    def tuning_id(self) -> str:
        """12 hex digits identifying WHICH job lists are installed (the measured durations are left out): two processes that
        print the same id launch the same lists for every layer."""
        return tuning_text_id(self.export_tuning())

    def reconstruct_dataset(self, splits, checkpoint_dir, batch_size=None, max_num=-1, test_again=False, seed=None):
        """Counterpart of ``reconstruct_dataset`` (gan.py:451-587) for in-memory splits.

        ``splits``: {'train'|'dev'|'test': (images [n,H,W,C] already in generator range, targets [n])}.
        Reconstructions are cached exactly where the reference caches them, so its readers find them:
        ``<checkpoint_dir>/recs_rr{R}_lr{lr:.5f}_iters{L}[_num{max_num}]/<split>/pickles/rec_{i:07d}_l{label}.pkl``
        (one array per image, gan.py:504-557; directory name parsed back by whitebox.py:252-257).  Pickles are
        written by ``py2pickle`` (protocol 2 + ``numpy.core`` module paths) so that the Python-2 reference can load them.  A batch whose pickles all exist is
        loaded instead of recomputed unless ``test_again``.  Returns {split: [recs, targets, originals]} (gan.py:585).
        """
        import pickle
        from . import py2pickle
        bs = int(batch_size or self.test_batch_size)
        if seed is None:
            seed = self._default_seed        # one seed per call: z0 rows are keyed by (seed, global row), not by how many
                                             # batches happened to be computed rather than loaded from the cache
        name = _config.rec_dir_name(int(self.rec_rr), float(self.rec_lr), int(self.rec_iters))
        if max_num > 0:
            name += "_num{:d}".format(max_num)
        rets = {}
        for split, (images, targets) in splits.items():
            out_dir = os.path.join(checkpoint_dir, name, split)
            pk_dir = os.path.join(out_dir, "pickles")
            os.makedirs(pk_dir, exist_ok=True)
            n = len(images) if max_num <= 0 else min(len(images), max_num)
            recs = []
            # a whole-split ``feats.pkl`` (gan.py:484-496) short-cuts the per-image pickles when present
            feats_path = os.path.join(out_dir, "feats.pkl")
            if os.path.exists(feats_path) and not test_again:
                try:
                    with open(feats_path, "rb") as f:
                        allr = np.asarray(pickle.load(f, encoding="latin1"), np.float32).reshape([-1] + list(self.image_dim))
                    if len(allr) >= n:
                        rets[split] = [allr[:n], np.asarray(targets[:n]), np.asarray(images[:n]).reshape([-1] + list(self.image_dim))]
                        continue
                except Exception:
                    pass
            # Caller batches of ``bs`` images decide what is cached (a batch whose pickles all exist is loaded, gan.py:504-557);
            # the batches that have to be computed are handed to the engine in runs of consecutive batches of up to
            # gan_defense.COALESCE_ROWS latent rows -- rows are independent without Batchnorm and z0 is keyed by (seed, global
            # row), so the pickles hold the same bits as one engine call per batch would write, several times sooner at the
            # reference's batch of 50 (tests/test_gpu_cache.py).  With USE_BN a batch is the unit of the statistics: no runs.
            from . import gan_defense as _gd
            per_call = bs if self.use_bn else _gd.engine_batch_images(bs, int(self.rec_rr), max(n, 1))
            path_of = lambda i: os.path.join(pk_dir, "rec_{:07d}_l{}.pkl".format(i, targets[i]))
            loaded = {}
            for start in range(0, n, bs):
                paths = [path_of(i) for i in range(start, min(n, start + bs))]
                if not test_again and all(os.path.exists(q) for q in paths):
                    try:
                        loaded[start] = np.stack([pickle.load(open(q, "rb"), encoding="latin1") for q in paths])
                    except Exception:
                        pass
            start = 0
            while start < n:
                if start in loaded:
                    recs.append(loaded[start])
                    start = min(n, start + bs)
                    continue
                end = min(n, start + bs)
                while end < n and end not in loaded and end - start + min(bs, n - end) <= per_call:
                    end = min(n, end + bs)
                batch = self.reconstruct(np.asarray(images[start:end], np.float32),
                                         seed=seed, first_row=start * int(self.rec_rr))
                batch = np.asarray(batch.cpu().numpy() if hasattr(batch, "cpu") else batch, np.float32)
                for i, r in zip(range(start, end), batch):
                    with open(path_of(i), "wb") as f:
                        py2pickle.dump(r, f)
                recs.append(batch)
                start = end
            all_recs = np.concatenate(recs).reshape([-1] + list(self.image_dim)) if recs else np.zeros([0] + list(self.image_dim), np.float32)
            rets[split] = [all_recs, np.asarray(targets[:n]), np.asarray(images[:n]).reshape([-1] + list(self.image_dim))]
        return rets

    def generate(self, z):
        """G(z): generator_fn(z, is_training=False) (gan.py:399)."""
        self._ensure_handle()
        torch = _torch()
        lib = self._lib()
        was_numpy = isinstance(z, np.ndarray)
        zz = self._to_device(z)
        N = int(zz.shape[0])
        H, W, Cc = self._arch.image_dim
        y = torch.empty(N, H, W, Cc, dtype=torch.float32, device=zz.device)
        with torch.cuda.device(zz.device):
            for r0 in range(0, N, 1 << 20):                   # dg_generate takes at most 2^20 rows per call
                n = min(1 << 20, N - r0)
                self._check(lib.dg_generate(self._handle, zz[r0:r0 + n].data_ptr(), n, y[r0:r0 + n].data_ptr(),
                                              torch.cuda.current_stream(zz.device).cuda_stream))
        return y.cpu().numpy() if was_numpy else y

    def loss_grad(self, images, z):
        """One loop body without the update: (y [B*R,H,W,C], loss [B*R], dz [B*R, latent])
        for images [B,...] and z [B*R, latent] (gan.py:409-417)."""
        self._ensure_handle()
        torch = _torch()
        lib = self._lib()
        was_numpy = isinstance(images, np.ndarray)
        x = self._to_device(images)
        zz = self._to_device(z)
        B = int(x.shape[0])
        R = int(zz.shape[0]) // B
        if R * B != int(zz.shape[0]):
            raise ValueError("z rows must be a multiple of the image count")
        H, W, Cc = self._arch.image_dim
        y = torch.empty(B * R, H, W, Cc, dtype=torch.float32, device=x.device)
        loss = torch.empty(B * R, dtype=torch.float32, device=x.device)
        dz = torch.empty_like(zz)
        with torch.cuda.device(x.device):
            self._check(lib.dg_loss_grad(self._handle, x.data_ptr(), zz.data_ptr(), B, R, y.data_ptr(),
                                           loss.data_ptr(), dz.data_ptr(),
                                           torch.cuda.current_stream(x.device).cuda_stream))
        if was_numpy:
            return y.cpu().numpy(), loss.cpu().numpy(), dz.cpu().numpy()
        return y, loss, dz

    def init_latents(self, n_rows, seed=0, first_row=0, std=None):
        self._ensure_handle()
        torch = _torch()
        lib = self._lib()
        dev = torch.device("cuda", self._device)
        z = torch.empty(int(n_rows), int(self.latent_dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            self._check(lib.dg_init_latents(self._handle, z.data_ptr(), int(n_rows), int(seed), int(first_row),
                                              float(std) if std else 0.0,
                                              torch.cuda.current_stream(dev).cuda_stream))
        return z

    # ------------------------------------------------------------------ the critic (gan.py:121-126, 167-199, 253-329)
    @property
    def critic(self):
        """The critic D (critic.mnist_discriminator at this model's net_dim and image_dim), built on first use; its weights come
        from load_discriminator, critic.init_like_tflib or critic.set_named_weights."""
        if self._critic is None:
            from . import critic as _critic
            if self._arch.arch_id == archs.ARCH_CELEBA:
                _critic.celeba_discriminator()
            self._critic = _critic.mnist_discriminator(net_dim=int(self.net_dim), input_shape=(None,) + tuple(self.image_dim),
                                                       use_bn=bool(self.use_bn))
            if self._device is not None:
                self._critic._device = int(self._device)
        return self._critic

    def _check_mode(self):
        if self.mode != 'wgan-gp':
            raise NotImplementedError("MODE %r is not implemented: only 'wgan-gp' (gan.py:167-199) is" % (self.mode,))

    def discriminator_fn(self, x):
        """D(x) [B]: the critic's one output per image (gan.py:121-126)."""
        self._ensure_handle()
        self.critic._device = self._device
        return self.critic.discriminate(x)

    def _critic_inputs(self, B, k, seed, gen):
        """Step k's fake batch and alpha: fake = G(z), z = the rows [k B, (k + 1) B) of the N(0, 1) draw keyed by ``seed``
        (init_latents with std 1: the training prior tf.random_normal of models/dataset_models.py:39-40, not the projection's
        sqrt(1 / latent));
        alpha = the next B uniforms of the device generator ``gen``."""
        torch = _torch()
        z = self.init_latents(B, seed=seed, first_row=k * B, std=1.0)
        return self.generate(z), torch.rand(B, generator=gen, device=z.device, dtype=torch.float32)

    def _alpha_generator(self, seed):
        torch = _torch()
        gen = torch.Generator(device=torch.device("cuda", self._device))
        gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        return gen

    def discriminator_cost(self, real, fake=None, alpha=None, seed=None, return_terms=False):
        """The reference's ``discriminator_cost`` fetch (its dev cost, gan.py:300-315): mean D(fake) - mean D(real) + lambda P.
        ``fake`` defaults to G(z), z ~ N(0, 1) [B, latent]; ``alpha`` to a seeded uniform draw made on the device.  Returns the
        cost (with ``return_terms``: cost, w, P)."""
        self._check_mode()
        self._ensure_handle()
        self.critic._device = self._device
        x = self._to_device(real)
        B = int(x.shape[0])
        if seed is None:
            seed = self._default_seed
        if fake is None or alpha is None:
            f, a = self._critic_inputs(B, 0, seed, self._alpha_generator(seed))
            fake = f if fake is None else fake
            alpha = a if alpha is None else alpha
        cost, _, _ = self.critic.gradient(x, self._to_device(fake), self._to_device(alpha), gp_lambda=float(self.gradient_penalty_lambda),
                                          penalty_axes=self.penalty_axes, sync=False)
        cost = cost.cpu().numpy()
        return tuple(float(c) for c in cost) if return_terms else float(cost[0])

    def critic_schedule(self, n_images, n_steps, seed):
        """[n_steps, batch_size] int64 image indices: a seeded permutation per epoch, cut into full batches (the tail of an epoch
        that does not fill a batch is dropped, as the reference's generators do)."""
        bs = int(self.batch_size)
        per_epoch = int(n_images) // bs
        if per_epoch < 1:
            raise ValueError("%d images do not fill one batch of %d" % (n_images, bs))
        rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
        rows = []
        while len(rows) < n_steps:
            perm = rs.permutation(int(n_images))
            rows.extend(perm[i * bs:(i + 1) * bs] for i in range(per_epoch))
        return np.asarray(rows[:n_steps], np.int64).reshape(n_steps, bs)

    def train(self, images, phase=None, train_iters=None, seed=None, learning_rate=1e-4, beta1=0.5, beta2=0.9):
        """The critic half of the reference's ``train`` (gan.py:253-329), which is all it runs for a ``phase`` other than None:
        ``train_iters`` iterations of ``critic_iters`` Adam steps (dg_critic_step; 1e-4, 0.5, 0.9) on successive batches of
        ``batch_size`` of ``images`` [n,H,W,C] (generator range), in the order of ``critic_schedule``.  Step k takes the fake batch
        and alpha of ``_critic_inputs(batch_size, k, seed, gen)``, gen one device generator seeded with ``seed``.  Nothing waits for
        the device inside the loop.  Returns [train_iters, 3]: each iteration's last cost, w and P (the reference plots the first).
        ``phase=None`` asks for generator steps as well: that loop is ``train_gan``; this entry keeps raising for it."""
        self._check_mode()
        if phase is None:
            raise NotImplementedError("train(phase=None) needs the generator step (a generator backward seeded from the critic, with "
                                      "weight gradients), which is not implemented; train(phase=...) trains the critic alone")
        torch = _torch()
        self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        self.critic._device = self._device
        iters = int(self.train_iters if train_iters is None else train_iters)
        ci, bs = int(self.critic_iters), int(self.batch_size)
        if seed is None:
            seed = self._default_seed
        x = self._to_device(images)
        sched = torch.from_numpy(self.critic_schedule(int(x.shape[0]), iters * ci, seed)).to(x.device)
        gen = self._alpha_generator(seed)
        costs = torch.empty(iters, 3, dtype=torch.float32, device=x.device)
        scratch = torch.empty(3, dtype=torch.float32, device=x.device)
        lam = float(self.gradient_penalty_lambda)
        for it in range(iters):
            for i in range(ci):
                k = it * ci + i
                fake, alpha = self._critic_inputs(bs, k, seed, gen)
                self.critic.step(x[sched[k]], fake, alpha, gp_lambda=lam, penalty_axes=self.penalty_axes, learning_rate=learning_rate,
                                 beta1=beta1, beta2=beta2, cost=costs[it] if i == ci - 1 else scratch)
        return costs.cpu().numpy()

    def save_discriminator(self, path: str) -> None:
        """An .npz of the critic: its parameters under their tflib names, Adam's moments as ``adam_m/<name>`` and ``adam_v/<name>``
        and the step count ``adam_t``."""
        c = self.critic
        arrays = dict(c.named_weights())
        t = 0
        for (wn, bn), ((mW, mb), (vW, vb), t) in zip(c.param_names, c.adam_state()):
            arrays["adam_m/" + wn], arrays["adam_m/" + bn] = mW, mb
            arrays["adam_v/" + wn], arrays["adam_v/" + bn] = vW, vb
        arrays["adam_t"] = np.asarray(t, np.int64)
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    def load_discriminator(self, path: str) -> None:
        """``path``: an .npz written by save_discriminator (or holding the parameters alone: Adam then starts afresh), or a
        reference checkpoint (directory, prefix or .index file) whose ``Discriminator.*`` variables are read by tf_checkpoint."""
        c = self.critic
        if self._device is not None:
            c._device = int(self._device)
        names = list(c.named_shapes())
        if path.endswith(".npz"):
            with np.load(path) as f:
                have = {k: f[k] for k in f.files}
        else:
            from . import tf_checkpoint
            have = tf_checkpoint.generator_weights(path, names)
        c.set_named_weights(have)
        lib = _native.load()
        if "adam_t" not in have:
            c.adam_reset()
            return
        for li, (wn, bn) in zip(c._param_layers, c.param_names):
            m = np.ascontiguousarray(np.concatenate([have["adam_m/" + wn].reshape(-1), have["adam_m/" + bn].reshape(-1)]), np.float32)
            v = np.ascontiguousarray(np.concatenate([have["adam_v/" + wn].reshape(-1), have["adam_v/" + bn].reshape(-1)]), np.float32)
            _native.check(lib.dg_clf_set_adam(c._handle, c._native_index[li], m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                              int(have["adam_t"]), 0))

    # ------------------------------------------------------------------ the generator step (gan.py:167-199, 273-293)
    def _check_trainable(self):
        """What the generator's training step is built for: MODE wgan-gp, the MNIST / F-MNIST generator, USE_BN False."""
        self._check_mode()
        if self._arch.arch_id == archs.ARCH_CELEBA:
            raise NotImplementedError("training the CelebA generator is not implemented: only the MNIST / F-MNIST generator is")
        if self.use_bn:
            raise NotImplementedError("training a Batchnorm generator (USE_BN: True) is not implemented")

    def weight_names(self):
        return list(archs.weight_shapes(self._arch, bool(self.use_bn)))

    def get_weights(self) -> Dict[str, np.ndarray]:
        """{tflib name: array in the reference layout}: the handle's current parameters (dg_get_weights), which training moves on
        the device; Batchnorm scale / offset, which nothing moves, as they were set."""
        self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        lib = self._lib()
        out = {}
        for name, shape in archs.weight_shapes(self._arch, bool(self.use_bn)).items():
            if ".BN" in name:
                out[name] = self._weights[name].copy()
                continue
            a = np.empty(shape, np.float32)
            self._check(lib.dg_get_weights(self._handle, name.encode(), a.ctypes.data_as(C.c_void_p), 0))
            out[name] = a
        return out

    def split_grads(self, flat) -> Dict[str, np.ndarray]:
        """dg_gen_param_gradient's flat gradient as {name: array}, in the order of archs.weight_shapes(arch, use_bn=False)."""
        out, off = {}, 0
        for name, shape in archs.weight_shapes(self._arch, False).items():
            n = int(np.prod(shape))
            out[name] = flat[off:off + n].reshape(shape)
            off += n
        return out

    def n_params(self) -> int:
        return sum(int(np.prod(s)) for s in archs.weight_shapes(self._arch, False).values())

    def _critic_seed(self, y):
        """(cost, dy) on the device for y = G(z) [B,H,W,C]: cost = -mean D(y) (gan.py:168) and dy = d cost / dy, the critic's input
        gradient for dlogits = -1/B (dg_clf_backward).  The critic's weights do not move."""
        torch = _torch()
        self.critic._device = self._device
        B = int(y.shape[0])
        cost = -self.critic.discriminate(y).mean()
        dl = torch.full((B, 1), -1.0 / B, dtype=torch.float32, device=y.device)
        return cost, self.critic.backward(y, dl)

    def generator_cost(self, z) -> float:
        """The reference's ``generator_cost`` fetch: -mean D(G(z)) (gan.py:168)."""
        self._check_trainable()
        self._ensure_handle()
        cost, _ = self._critic_seed(self.generate(self._to_device(z)))
        return float(cost.cpu())

    def _gen_inputs(self, z, dy):
        self._check_trainable()
        self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        zz = self._to_device(z)
        if zz.dim() != 2 or int(zz.shape[1]) != int(self.latent_dim) or int(zz.shape[0]) < 1:
            raise ValueError("z must be [N,%d] with N >= 1, got %r" % (int(self.latent_dim), tuple(zz.shape)))
        N = int(zz.shape[0])
        cost = None
        if dy is None:
            cost, dy = self._critic_seed(self.generate(zz))
        dy = self._to_device(dy)
        if int(dy.numel()) != N * self._arch.pixels:
            raise ValueError("dy must be [%d,%d,%d,%d], got %r" % ((N,) + tuple(self._arch.image_dim) + (tuple(dy.shape),)))
        return zz, dy, N, cost

    def generator_gradient(self, z, dy=None, sync=True):
        """(cost, {name: gradient}, dz) of the generator at ``z`` [N, latent] (dg_gen_param_gradient).  ``dy`` [N,H,W,C] is the
        gradient with respect to G(z); None means the critic's seed, the composition the reference's ``gen_train_op`` differentiates:
        cost = -mean D(G(z)), dy = dg_clf_backward on the critic at G(z) with dlogits = -1/N (cost is None for an explicit ``dy``).
        ``sync``: NumPy results; otherwise (cost tensor, flat gradient tensor, dz tensor) on the device and no wait."""
        torch = _torch()
        zz, dy, N, cost = self._gen_inputs(z, dy)
        grads = torch.empty(self.n_params(), dtype=torch.float32, device=zz.device)
        dz = torch.empty_like(zz)
        with torch.cuda.device(zz.device):
            self._check(self._lib().dg_gen_param_gradient(self._handle, zz.data_ptr(), dy.data_ptr(), N, grads.data_ptr(), None,
                                                          dz.data_ptr(), torch.cuda.current_stream(zz.device).cuda_stream))
        if not sync:
            return cost, grads, dz
        return (None if cost is None else float(cost.cpu())), self.split_grads(grads.cpu().numpy()), dz.cpu().numpy()

    def generator_step(self, z, dy=None, learning_rate=1e-4, beta1=0.5, beta2=0.9):
        """One Adam step of the generator (dg_gen_step; the reference's gen_train_op: 1e-4, 0.5, 0.9) on the gradient of
        ``generator_gradient(z, dy)``; every derived weight layout of the engine follows on the device.  Returns the cost before the
        update as a device tensor without waiting (None for an explicit ``dy``)."""
        torch = _torch()
        zz, dy, N, cost = self._gen_inputs(z, dy)
        with torch.cuda.device(zz.device):
            self._check(self._lib().dg_gen_step(self._handle, zz.data_ptr(), dy.data_ptr(), N, float(learning_rate), float(beta1),
                                                float(beta2), torch.cuda.current_stream(zz.device).cuda_stream))
        return cost

    def generator_adam_reset(self) -> None:
        self._check_trainable()
        self._ensure_handle()
        self._check(self._lib().dg_gen_adam_reset(self._handle))

    def generator_adam_state(self):
        """({name: m}, {name: v}, t) of the generator's optimiser (dg_gen_get_adam)."""
        self._check_trainable()
        self._ensure_handle()
        lib = self._lib()
        m, v, t = {}, {}, C.c_int64(0)
        for name, shape in archs.weight_shapes(self._arch, False).items():
            m[name], v[name] = np.empty(shape, np.float32), np.empty(shape, np.float32)
            self._check(lib.dg_gen_get_adam(self._handle, name.encode(), m[name].ctypes.data_as(C.c_void_p),
                                            v[name].ctypes.data_as(C.c_void_p), C.byref(t), 0))
        return m, v, int(t.value)

    def _set_generator_adam(self, m, v, t) -> None:
        lib = self._lib()
        for name in archs.weight_shapes(self._arch, False):
            mm, vv = np.ascontiguousarray(m[name], np.float32), np.ascontiguousarray(v[name], np.float32)
            self._check(lib.dg_gen_set_adam(self._handle, name.encode(), mm.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p),
                                            int(t), 0))

    def save_generator(self, path: str) -> None:
        """An .npz of the generator: its parameters under their tflib names (what load_generator and --init_path read), Adam's moments
        as ``adam_m/<name>`` and ``adam_v/<name>`` and the step count ``adam_t`` (what load_generator_state also restores)."""
        arrays = dict(self.get_weights())
        m, v, t = self.generator_adam_state()
        arrays.update(generator_state_arrays(m, v, t))
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    def load_generator_state(self, path: str) -> None:
        """load_generator(path) and the optimiser with it: Adam's moments and step count when the .npz holds them (save_generator),
        a fresh optimiser when not.  (load_generator itself keeps ignoring those keys: it works without a device.)"""
        self._check_trainable()
        self.load_generator(path)
        self._ensure_handle()
        state = None
        if path.endswith(".npz") or os.path.isdir(path):
            p = os.path.join(path, "generator.npz") if os.path.isdir(path) else path
            if os.path.exists(p):
                with np.load(p) as f:
                    state = split_generator_state({k: f[k] for k in f.files}, list(archs.weight_shapes(self._arch, False)))
        if state is None:
            self.generator_adam_reset()
        else:
            self._set_generator_adam(*state)

    def train_gan(self, images, train_iters=None, seed=None, learning_rate=1e-4, beta1=0.5, beta2=0.9, start_iter=0):
        """What the reference's ``train(phase=None)`` does (gan.py:273-293): ``train_iters`` iterations, every one after the first
        starting with ONE generator step (``generator_step`` with the critic's seed) followed by ``critic_iters`` critic steps exactly
        as ``train(phase="disc")`` schedules them -- the same ``critic_schedule``, ``_critic_inputs`` and alpha stream, k the running
        critic-step index -- whose fake batches come from the generator's CURRENT weights.  The generator step of iteration ``it``
        takes z = init_latents(batch_size, seed=seed + 1, first_row=it * batch_size, std=1.0).  Nothing waits for the device inside the
        loop.  ``start_iter`` continues a run: the iterations [start_iter, start_iter + train_iters) of the run that began at 0 with
        the same ``seed`` (the schedule and the alpha stream are advanced past the earlier ones; weights and optimisers are the
        caller's to restore).  Returns [train_iters, 4]: each iteration's last critic cost, w and P, and the cost of its generator step
        (NaN for iteration 0, which has none)."""
        self._check_trainable()
        torch = _torch()
        self._ensure_handle()
        if not self.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        self.critic._device = self._device
        iters = int(self.train_iters if train_iters is None else train_iters)
        ci, bs, first = int(self.critic_iters), int(self.batch_size), int(start_iter)
        if seed is None:
            seed = self._default_seed
        x = self._to_device(images)
        sched = torch.from_numpy(self.critic_schedule(int(x.shape[0]), (first + iters) * ci, seed)).to(x.device)
        gen = self._alpha_generator(seed)
        for _ in range(first * ci):                   # the alphas of the iterations already run
            torch.rand(bs, generator=gen, device=x.device, dtype=torch.float32)
        costs = torch.full((iters, 4), float("nan"), dtype=torch.float32, device=x.device)
        scratch = torch.empty(3, dtype=torch.float32, device=x.device)
        lam = float(self.gradient_penalty_lambda)
        for it, k0, gen_step in gan_iteration_plan(first, iters, ci):
            if gen_step:
                z = self.init_latents(bs, seed=seed + 1, first_row=it * bs, std=1.0)
                costs[it - first, 3] = self.generator_step(z, learning_rate=learning_rate, beta1=beta1, beta2=beta2)
            for i in range(ci):
                k = k0 + i
                fake, alpha = self._critic_inputs(bs, k, seed, gen)
                self.critic.step(x[sched[k]], fake, alpha, gp_lambda=lam, penalty_axes=self.penalty_axes, learning_rate=learning_rate,
                                 beta1=beta1, beta2=beta2, cost=costs[it - first, :3] if i == ci - 1 else scratch)
        return costs.cpu().numpy()

    # ------------------------------------------------------------------ measurement hooks
    def set_option(self, key: str, value) -> None:
        self._ensure_handle()
        self._check(self._lib().dg_set_option(self._handle, key.encode(), str(value).encode()))

    def profile_enable(self, stride: int) -> None:
        self._ensure_handle()
        self._check(self._lib().dg_profile_enable(self._handle, int(stride)))

    def profile_reset(self) -> None:
        self._ensure_handle()
        self._check(self._lib().dg_profile_reset(self._handle))

    def profile_read(self):
        """[{name, launches, ms, flops}] per kernel family since the last reset."""
        self._ensure_handle()
        lib = self._lib()
        n = lib.dg_profile_count(self._handle)
        out = []
        for i in range(max(n, 0)):
            name = C.create_string_buffer(64)
            launches = C.c_int64()
            ms = C.c_double()
            fl = C.c_double()
            self._check(lib.dg_profile_read(self._handle, i, name, 64, C.byref(launches), C.byref(ms), C.byref(fl)))
            out.append({"name": name.value.decode(), "launches": launches.value, "ms": ms.value, "flops": fl.value})
        return out

    def debug_read(self, what: str, n: int):
        self._ensure_handle()
        torch = _torch()
        dev = torch.device("cuda", self._device)
        torch.cuda.synchronize(dev)
        t = torch.empty(int(n), dtype=torch.float32, device=dev)
        got = self._lib().dg_debug_read(self._handle, what.encode(), t.data_ptr(), int(n))
        if got < 0:
            self._check(int(got))
        return t[:got]


def gan_iteration_plan(start_iter: int, train_iters: int, critic_iters: int):
    """The bookkeeping of ``train_gan``: per iteration (it, k0, generator_step) -- the iteration's index in the whole run, the running
    index of its first critic step, and whether it starts with a generator step (every iteration but the run's first, gan.py:279)."""
    return [(it, it * int(critic_iters), it > 0) for it in range(int(start_iter), int(start_iter) + int(train_iters))]


def generator_state_arrays(m: Dict[str, np.ndarray], v: Dict[str, np.ndarray], t: int) -> Dict[str, np.ndarray]:
    """The optimiser's entries of save_generator's .npz: adam_m/<name>, adam_v/<name>, adam_t."""
    out = {}
    for name in m:
        out["adam_m/" + name], out["adam_v/" + name] = m[name], v[name]
    out["adam_t"] = np.asarray(int(t), np.int64)
    return out


def split_generator_state(arrays: Dict[str, np.ndarray], names):
    """(m, v, t) from the arrays of a save_generator .npz, or None when it holds the parameters alone."""
    if "adam_t" not in arrays:
        return None
    missing = [p + n for n in names for p in ("adam_m/", "adam_v/") if p + n not in arrays]
    if missing:
        raise ValueError("optimiser state lacks %s" % ", ".join(missing))
    return ({n: np.asarray(arrays["adam_m/" + n], np.float32) for n in names},
            {n: np.asarray(arrays["adam_v/" + n], np.float32) for n in names}, int(arrays["adam_t"]))


def tuning_text_id(text: str) -> str:
    """12 hex digits naming the job lists a dg_export_tuning text describes.  A record is
    ``op n_rows min_level slack snake xcd_order xcd_head n_jobs measured_us [taper [prio [pair_kernel]]]`` (dg_plan.cpp format_tune_record):
    every field but ``measured_us`` (index 8, informational: two timings of the same list differ) enters the id, the taper
    and the priority mode -- which do change the list -- included; fields an older text lacks count as 0."""
    import hashlib
    lines = text.strip().splitlines()
    keys = []
    for ln in lines[1:]:
        f = ln.split()
        if len(f) < 9:
            keys.append(" ".join(f))         # not a record this build writes: hashed as it is
            continue
        taper = f[9] if len(f) > 9 else "0"
        prio = f[10] if len(f) > 10 else "0"                  # eleventh field (round 5): wave priorities by job length
        pairk = f[11] if len(f) > 11 else "0"                 # twelfth: the list runs the PAIR instantiation of the kernel
        keys.append(" ".join(f[:8] + ["%.17g" % float(taper), str(int(prio)), str(int(pairk))]))
    return hashlib.sha256("\n".join(sorted(keys) if keys else lines).encode()).hexdigest()[:12]


class ReconstructionLayer(object):
    """The classifier-side wrapper of the reference (utils/network_builder.py:239-271): a layer whose forward pass
    is the Defense-GAN projection.  ``model`` is a DefenseGANBase; ``z_init`` an optional fixed [B*R, latent] init
    (whitebox.py --same_init); the reference's ``reconstructor_id=123`` only named TF variables."""

    def __init__(self, model, z_init, input_shape, batch_size):
        self.z_init = z_init
        self.rec_model = model
        self.input_shape = input_shape
        self.batch_size = batch_size
        self.rec = None

    def set_input_shape(self, shape):
        self.input_shape = shape
        self.output_shape = shape

    def get_output_shape(self):
        return self.output_shape

    def fprop(self, x):
        z = self.z_init
        if z is not None:
            z = z[: len(x) * int(self.rec_model.rec_rr)]
        self.rec = self.rec_model.reconstruct(x, batch_size=self.batch_size, back_prop=True, z_init_val=z,
                                              reconstructor_id=123)
        return self.rec


class MnistDefenseGAN(DefenseGANBase):          # gan.py:649-685
    arch_name = "mnist"


class FmnistDefenseDefenseGAN(MnistDefenseGAN):  # gan.py:688-698 (same generator, other weights; name sic)
    arch_name = "f-mnist"


class CelebADefenseGAN(DefenseGANBase):         # gan.py:717-765
    arch_name = "celeba"


# whitebox.py / blackbox.py pick the class by FLAGS.dataset_name
dataset_gan_dict = {
    "mnist": MnistDefenseGAN,
    "f-mnist": FmnistDefenseDefenseGAN,
    "celeba": CelebADefenseGAN,
}


def gan_from_config(cfg_path: str, test_mode: bool = True, **overrides) -> DefenseGANBase:
    """``GAN(cfg=load_config(path), test_mode=True)`` as whitebox.py:239-244 does."""
    cfg = _config.load_config(cfg_path)
    cls = dataset_gan_dict[str(cfg.get("DATASET_NAME", overrides.get("dataset_name", "mnist"))).lower()]
    return cls(cfg=cfg, test_mode=test_mode, **overrides)
