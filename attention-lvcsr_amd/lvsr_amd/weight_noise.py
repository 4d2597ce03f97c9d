"""Adaptive weight noise (Graves, NIPS 2011): the reference's `apply_adaptive_noise` (lvsr/graph.py:71-249, wired at
lvsr/main.py:425-456) on the flat parameter layout.

Every parameter of the store is noisy: the store's names are the reference's `Model.get_parameter_dict()` of the cost graph
(spec.parameter_shapes), and each of them reaches the training cost, so `cg.parameters` (main.py:431-437) covers them all.
The trainer owns theta = [mu | ls2] (each half in the store's layout); a step draws the noisy weights into `store.flat`
(csrc/weight_noise.hip: lvsr_wnoise_sample), runs forward and backward there, rewrites the gradient (lvsr_wnoise_grad) and lets
the fused optimiser update means and log-variances together; `store.flat` gets the means back behind the optimiser.

Checkpoints: the log-variances belong to the brick `adaptive_noise` (graph.py:24-39) and are named after their parameter
(`__get_name`, :57-68: the brick path without the leading '/', a '.', the parameter's name), so Blocks' Model.get_parameter_dict
files the log-variance of `/recognizer/X.W` as `/adaptive_noise.recognizer/X.W` (`|adaptive_noise.recognizer|X.W` in the tar).
"""
import ctypes

import numpy
import torch

SCALE = 2048.0                       # log_sigma_scale, graph.py:159
PREFIX = "/adaptive_noise."
STATS = 8 + 4 * 1024                 # include/lvsr_hip.h lvsr_wnoise_args.stats
DEFAULTS = dict(model_cost_coefficient=1.0, init_sigma=1e-6, seed=None)


def noise_name(param):
    """'/recognizer/X.W' -> '/adaptive_noise.recognizer/X.W'."""
    assert param.startswith("/")
    return PREFIX + param[1:]


def param_name(name):
    """Inverse of noise_name."""
    assert name.startswith(PREFIX)
    return "/" + name[len(PREFIX):]


def is_noise_name(name):
    return name.startswith(PREFIX)


def initial_ls2(init_sigma):
    """graph.py:171-173: log(init_sigma) * 2 / log_sigma_scale, as float32."""
    return numpy.float32(numpy.log(init_sigma) * 2.0 / SCALE)


def settings(adaptive_noise):
    """`regularization.adaptive_noise` (a mapping, or True for the defaults) -> the full settings, or None when it is off."""
    if not adaptive_noise:
        return None
    conf = dict(DEFAULTS)
    if isinstance(adaptive_noise, dict):
        unknown = set(adaptive_noise) - set(DEFAULTS)
        if unknown:
            raise ValueError("unknown adaptive_noise settings %s (known: %s)" % (sorted(unknown), sorted(DEFAULTS)))
        conf.update(adaptive_noise)
    return conf


class WeightNoise(object):
    """Device state of adaptive noise for one trainer: theta = [mu | ls2], its gradient, the step counter and the statistics."""

    def __init__(self, recognizer, segments, num_examples, model_cost_coefficient=1.0, init_sigma=1e-6, seed=None):
        st = recognizer.store
        self.rec, self.store, self.lib = recognizer, st, recognizer.lib
        self.coef, self.init_sigma, self.num_examples = float(model_cost_coefficient), float(init_sigma), float(num_examples)
        self.seed = 1 if seed is None else int(seed)        # Blocks' config.default_seed
        if not self.num_examples > 0:
            raise ValueError("adaptive noise needs the number of training examples (got %r)" % (num_examples,))
        n = st.flat.numel()
        self.n = n
        dev = st.device
        self.segments = segments                             # the store's tensors (rows of the trainer's segment table)
        self.theta = torch.zeros(2 * n, dtype=torch.float32, device=dev)
        self.gtheta = torch.zeros(2 * n, dtype=torch.float32, device=dev)
        self.mu, self.ls2 = self.theta[:n], self.theta[n:]
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(STATS, dtype=torch.float64, device=dev)
        self.mu.copy_(st.flat)
        init = initial_ls2(self.init_sigma)
        stored = getattr(recognizer, "noise_values", None) or {}
        self.adopted = []
        for name, (off, cnt) in st.offsets.items():
            v = stored.get(name)
            if v is not None:
                self.ls2[off:off + cnt].copy_(torch.from_numpy(numpy.ascontiguousarray(v, numpy.float32).reshape(-1)))
                self.adopted.append(name)
            else:
                self.ls2[off:off + cnt].fill_(float(init))

    def key(self):
        return ("adaptive_noise", self.coef, self.init_sigma, self.num_examples, self.seed)

    def _args(self, grad=None, grad_scale=1.0):
        return self.lib.make("lvsr_wnoise_args", mu=self.mu, ls2=self.ls2, noisy=self.store.flat, segments=self.segments,
                             nseg=int(self.segments.shape[0]), n=self.n, seed=self.seed, counter=self.counter, stats=self.stats,
                             grad=grad, grad_scale=float(grad_scale), coef=self.coef, num_examples=self.num_examples,
                             gtheta=self.gtheta)

    def enqueue_sample(self):
        """Head of a step: the noisy weights into store.flat, prior and model cost into stats."""
        a = self._args()
        self.lib.call("lvsr_wnoise_sample", self.lib.stream_for(self.store.flat), ctypes.byref(a))

    def enqueue_grad(self, grad, grad_scale):
        """Behind the (all-reduced) backward pass: gtheta = [d/dmu | d/dls2]; advances the step counter."""
        a = self._args(grad, grad_scale)
        self.lib.call("lvsr_wnoise_grad", self.lib.stream_for(self.store.flat), ctypes.byref(a))

    def publish(self):
        """store.flat <- the means (behind the optimiser, skipped step or not)."""
        self.store.flat.copy_(self.mu)

    def ls2_values(self):
        """{'/adaptive_noise.recognizer/...': ndarray} of the current log-variances (synchronises)."""
        host = self.ls2.detach().cpu().numpy()
        return {noise_name(k): host[o:o + c].reshape(self.store.shapes[k]).copy() for k, (o, c) in self.store.offsets.items()}

    def observables(self):
        """The last step's model cost, prior mean and prior variance (synchronises)."""
        s = self.stats[4:7].cpu().numpy()
        return dict(model_cost=float(s[2]), model_prior_mean=float(s[0]), model_prior_variance=float(s[1]))
