from .encoder import GaussianEncoderBase
from .enc_lstm import LSTMEncoder, VarLSTMEncoder
from .enc_resnet_v2 import ResNetEncoderV2

__all__ = ["GaussianEncoderBase", "LSTMEncoder", "VarLSTMEncoder", "ResNetEncoderV2"]
