"""The life of a native handle, the same for the seven classes that own a model (gprc_amd._native.Handle): use, close() twice, a use
after close() refused with the class's own text, the `with` form, and an object whose constructor raised collected in silence.
Every failing case fails in a Python argument check or on a null handle, which the library refuses before it touches the device."""
import gc
import sys

import numpy as np
import pytest

import gprc_amd
from gprc_amd import GPC, GPR, BatchGPR, GprcError, IterativeGPR, LocalGPR, SamplePaths, SparseGPR, cov_func, sqrexp

pytestmark = pytest.mark.gpu

N, D = 16, 2
_rng = np.random.default_rng(3)
X = np.asfortranarray(_rng.uniform(-1, 1, (D, N)))
Y = np.sin(2 * X[0]) + 0.5 * X[1] + 0.05 * _rng.standard_normal(N)
XS = np.asfortranarray(_rng.uniform(-1, 1, (D, 5)))
K = cov_func(sqrexp, l=0.8)


def _paths():
    with GPR(X, Y, 0.1, K) as g:
        return g.sample_paths(2, 8, rng=np.random.default_rng(1))     # the paths outlive the model


# class -> (make a model, use it once, what a use after close() says, constructor arguments refused before any native call)
CASES = {
    GPR: (lambda: GPR(X, Y, 0.1, K), lambda m: m.predict(XS), "predict: not a GPR model", ((X, Y[:3], 0.1, K), {})),
    GPC: (lambda: GPC(X, np.sign(Y), K, reference_stop=False), lambda m: m.predict_class(XS), "predict_class: not a GPC model", ((X, np.sign(Y)[:3], K), {})),
    SparseGPR: (lambda: SparseGPR(X, Y, 0.1, K, X[:, :4]), lambda m: m.predict(XS), "model already closed", ((X, Y[:3], 0.1, K, X[:, :4]), {})),
    IterativeGPR: (lambda: IterativeGPR(X, Y, 0.1, K), lambda m: m.predict(XS), "model already closed", ((X, Y[:3], 0.1, K), {})),
    BatchGPR: (lambda: BatchGPR(X, Y, 0.1, "sqrexp", [[0.8], [1.2]]), lambda m: m.predict(XS), "the batch has been closed",
               ((X, Y, 0.1, "sqrexp", np.empty((0, 1))), {})),
    LocalGPR: (lambda: LocalGPR(X, Y, 0.1, K, m=4), lambda m: m.predict(XS), "model already closed", ((X, Y, 0.1, K), {"m": 0})),
    SamplePaths: (_paths, lambda m: m.paths(XS), "sample paths already closed", ((None, D, None, None, np.zeros(3), None), {})),   # w is no matrix
}


def used(out):
    """every number a use returned is finite"""
    return all(np.all(np.isfinite(a)) for a in (out if isinstance(out, (tuple, list)) else [out]) if a is not None)


@pytest.mark.parametrize("cls", list(CASES), ids=lambda c: c.__name__)
def test_the_life_of_a_handle(cls, monkeypatch):
    make, use, closed_text, (bad_args, bad_kw) = CASES[cls]
    assert issubclass(cls, gprc_amd._native.Handle)
    m = make()
    assert used(use(m))
    m.close()
    m.close()                                                    # a no-op
    with pytest.raises(GprcError) as e:
        use(m)
    assert e.value.message == closed_text and e.value.status == gprc_amd._native.ERR_ARG
    with make() as w:
        assert used(use(w))
    with pytest.raises(GprcError) as e:
        use(w)
    assert e.value.message == closed_text
    w.close()                                                    # after the with form too

    unraisable = []
    monkeypatch.setattr(sys, "unraisablehook", unraisable.append)
    half = cls.__new__(cls)                                      # the object Python is left with when the constructor raises
    with pytest.raises((ValueError, TypeError)):
        half.__init__(*bad_args, **bad_kw)
    half.close()
    half.__del__()
    del half
    with pytest.raises((ValueError, TypeError)):
        cls(*bad_args, **bad_kw)                                 # the ordinary spelling: the half-made object is collected here
    gc.collect()
    assert unraisable == []
