"""Mirror of the reference's ``training`` package for the pieces on the hot path
(training/pixelwise_nllloss.py; metrics of training/train_ubresnet2018_wlarcv2.py:509-566)."""


def __getattr__(name):
    # exported lazily: importing the package alone loads neither torch nor a library
    if name == "PixelWiseFocalLoss":
        from .pixelwise_focalloss import PixelWiseFocalLoss
        return PixelWiseFocalLoss
    if name in ("PixelWiseDiceLoss", "WeightedSumLoss"):
        from . import pixelwise_diceloss
        return getattr(pixelwise_diceloss, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
