from .basics import SpectralConv1d, SpectralConv2d, SpectralConv3d  # noqa: F401
from .fourier1d import FNO1d  # noqa: F401
from .fourier2d import FNO2d  # noqa: F401
from .pinobserver import MultiplicativeNet, PINObserver2d, PINObserverFullField, PlanePredHead, PolicyModel2D  # noqa: F401
