"""The label codecs of the two recognition heads (attn.AttnConvertor, ctc.CTCConvertor); what they share is base.BaseConvertor."""
from .base import checked_beam_width, nbest_lists  # noqa: F401
