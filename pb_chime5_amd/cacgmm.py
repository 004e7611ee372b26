"""The fitted mixture model as an object: pb_bss's ``CACGMM`` / ``CACGMMTrainer`` for all
frequencies at once, on the GPU (``gss_cacgmm_fit`` / ``gss_cacgmm_predict``).

The reference runs its schedule as three calls (core.py:180-202): ``fit(initialization=array)``,
``fit(initialization=model)``, ``model.predict(y[, source_activity_mask])``.  With the model in
hand a caller can fit on one stretch of frames and predict another, continue a fit, score frames
under a model and carry a model from one call to the next.

Layouts are those of ``ops.cacgmm_posteriors_guided``: Obs (D,T,F), tables (K,T) or (K,T,F),
posterior (K,T,F), log-likelihood (T,F).
"""
import numpy as np


class CACGMM:
    """A fitted model on the host: ``precision`` (F,K,D,D) complex128, the Hermitian B_k^-1;
    ``log_determinant`` (F,K), ln det B_k; ``weight`` (F,K), pi_k.

    Posteriors and log-likelihood depend on (precision, log_determinant) only through
    ``-D ln(y^H B^-1 y) - ln det B``: B_k may carry any positive scale.  A model that comes out
    of a fit holds the bits the EM left (so predict and a further fit continue exactly), which
    for most classes is NOT pb_bss's scale (largest eigenvalue of B_k = 1); ``normalized()``
    gives that form."""

    def __init__(self, precision, log_determinant, weight):
        precision = np.asarray(precision)
        log_determinant = np.asarray(log_determinant)
        weight = np.asarray(weight)
        if precision.ndim != 4 or precision.shape[-1] != precision.shape[-2]:
            raise ValueError(f'precision: shape {precision.shape} is not (F,K,D,D)')
        if not np.iscomplexobj(precision):
            raise ValueError(f'precision: dtype {precision.dtype} is not complex')
        for name, a in (('log_determinant', log_determinant), ('weight', weight)):
            if a.shape != precision.shape[:2]:
                raise ValueError(f'{name}: shape {a.shape} is not (F,K) = {precision.shape[:2]}')
            if a.dtype.kind not in 'fiu':
                raise ValueError(f'{name}: dtype {a.dtype} is not real')
        self.precision = np.ascontiguousarray(precision, dtype=np.complex128)
        self.log_determinant = np.ascontiguousarray(log_determinant, dtype=np.float64)
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)

    @property
    def shape(self):
        """(F, K, D)"""
        return self.precision.shape[:3]

    def check_observation(self, Obs):
        """ValueError unless Obs is (D,T,F) of this model's D and F."""
        shape = np.shape(Obs)
        F, _, D = self.shape
        if len(shape) != 3:
            raise ValueError(f'Obs: shape {shape} is not (D,T,F)')
        if shape[0] != D or shape[2] != F:
            raise ValueError(f'Obs: shape {shape} is (D,T,F) with D = {shape[0]}, F = {shape[2]} but '
                             f'the model has D = {D}, F = {F}')

    def predict(self, Obs, source_activity_mask=None, *, ctx=None):
        """``CACGMM.predict`` (affiliation_eps = 0): Obs (D,T,F) of any T -> posterior (K,T,F)."""
        from . import ops
        return ops.cacgmm_predict(self, Obs, source_activity_mask, ctx=ctx)

    def log_likelihood(self, Obs, source_activity_mask=None, *, ctx=None):
        """ln sum_k pi_k m_kt p_k(y_t) per frame and frequency, (T,F), without the constant
        ln((D-1)! / (2 pi^D)) of the density; -inf where the mask turns every class off."""
        from . import ops
        return ops.cacgmm_log_likelihood(self, Obs, source_activity_mask, ctx=ctx)

    def normalized(self):
        """The same model at pb_bss's scale: the largest eigenvalue of every B_k is 1, i.e. the
        smallest of the precision.  That eigenvalue is known from the precision to
        ``eps * cond(B_k)`` only; posteriors do not depend on the scale at all."""
        D = self.precision.shape[-1]
        c = 1.0 / np.linalg.eigvalsh(self.precision)[..., 0]
        return CACGMM(self.precision * c[..., None, None], self.log_determinant - D * np.log(c),
                      self.weight)

    def permuted(self, mapping):
        """The model with its classes renumbered per frequency, on the host: class k of frequency
        f of the result is class ``mapping[f, k]`` of this one, so that its ``predict`` gives
        this model's posteriors gathered the same way.  ``mapping`` (F,K) integers, every row a
        permutation of 0..K-1 (`ops.align_posteriors` returns one); ValueError otherwise.
        `ops.cacgmm_model_permute` is the device version."""
        from . import ops
        F, K, _ = self.shape
        mapping = ops.check_mapping(mapping, F, K)
        rows = np.arange(F)[:, None]
        return CACGMM(self.precision[rows, mapping], self.log_determinant[rows, mapping],
                      self.weight[rows, mapping])

    def save(self, path):
        """np.savez of the three arrays (no pickle)."""
        np.savez(path, precision=self.precision, log_determinant=self.log_determinant,
                 weight=self.weight)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as data:
            return cls(data['precision'], data['log_determinant'], data['weight'])


class CACGMMTrainer:
    """pb_bss ``CACGMMTrainer``: ``fit(Obs, initialization, iterations, source_activity_mask)``
    with ``initialization`` an affiliation array (K,T) / (K,T,F) -- ``iterations`` M-steps -- or
    a ``CACGMM`` -- ``iterations`` E-step + M-step pairs from it."""

    def fit(self, Obs, initialization, iterations=100, source_activity_mask=None, *, ctx=None):
        from . import ops
        if isinstance(initialization, CACGMM):
            return ops.cacgmm_fit(Obs, None, source_activity_mask, iterations,
                                  model=initialization, ctx=ctx)
        if initialization is None:
            raise ValueError('initialization: an affiliation array or a CACGMM, not None')
        return ops.cacgmm_fit(Obs, initialization, source_activity_mask, iterations, ctx=ctx)
