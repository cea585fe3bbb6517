"""Open3D ``pipelines.registration`` robust kernels: ``L2Loss``, ``L1Loss``, ``HuberLoss(k)``,
``CauchyLoss(k)``, ``GMLoss(k)``, ``TukeyLoss(k)``.

Pass one as ``kernel=`` to ``registration_icp`` (point-to-plane:
``TransformationEstimationPointToPlane(kernel)``) or ``registration_generalized_icp``
(``TransformationEstimationForGeneralizedICP(epsilon, kernel)``): every residual r then enters the
normal equations with the weight ``kernel.weight(r)`` (Open3D 0.19 ``RobustKernel.cpp``; the device
code, csrc/robust.hip, evaluates the same fp64 operations in the same order).  ``L2Loss`` — or no
kernel — is the unweighted estimator.
"""

from __future__ import annotations

import numpy as np

from m3d import _lib

__all__ = ["L2Loss", "L1Loss", "HuberLoss", "CauchyLoss", "GMLoss", "TukeyLoss"]


class RobustKernel:
    """Base class: ``kind`` is the library's M3D_KERNEL_* constant."""

    kind = _lib.ROBUST_L2

    def weight(self, residual):
        raise NotImplementedError

    def __repr__(self):
        k = getattr(self, "k", None)
        return f"{type(self).__name__}()" if k is None else f"{type(self).__name__}(k={k!r})"


class _Scaled(RobustKernel):
    def __init__(self, k):
        self.k = float(k)


class L2Loss(RobustKernel):
    kind = _lib.ROBUST_L2

    def weight(self, residual):
        return np.ones_like(np.asarray(residual, np.float64))


class L1Loss(RobustKernel):
    kind = _lib.ROBUST_L1

    def weight(self, residual):
        with np.errstate(divide="ignore"):
            return 1.0 / np.abs(np.asarray(residual, np.float64))


class HuberLoss(_Scaled):
    kind = _lib.ROBUST_HUBER

    def weight(self, residual):
        return self.k / np.maximum(np.abs(np.asarray(residual, np.float64)), self.k)


class CauchyLoss(_Scaled):
    kind = _lib.ROBUST_CAUCHY

    def weight(self, residual):
        r = np.asarray(residual, np.float64)
        return 1.0 / (1.0 + (r / self.k) * (r / self.k))


class GMLoss(_Scaled):
    kind = _lib.ROBUST_GM

    def weight(self, residual):
        r = np.asarray(residual, np.float64)
        return self.k / ((self.k + r * r) * (self.k + r * r))


class TukeyLoss(_Scaled):
    kind = _lib.ROBUST_TUKEY

    def weight(self, residual):
        t = np.minimum(1.0, np.abs(np.asarray(residual, np.float64) / self.k))
        u = 1.0 - t * t
        return u * u
