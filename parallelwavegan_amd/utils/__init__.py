from .utils import *  # noqa: F401,F403
from .precision import get_inference_precision, set_inference_precision  # noqa: E402,F401
from .streaming import (CausalStream, ChunkedSynthesizer, LookaheadStream, MelGANLookaheadStream,  # noqa: E402,F401
                        MelGANRaggedSynthesizer, MelGANStreamPool, PWGLookaheadStream, PWGRaggedSynthesizer, PWGStream, PWGStreamPool,
                        RaggedSynthesizer, StreamPool, StyleMelGANRaggedSynthesizer)
