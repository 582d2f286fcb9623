from .decoder import DecoderBase
from .dec_lstm import LSTMDecoder, VarLSTMDecoder
from .dec_pixelcnn_v2 import PixelCNNDecoderV2

__all__ = ["DecoderBase", "LSTMDecoder", "VarLSTMDecoder", "PixelCNNDecoderV2"]
