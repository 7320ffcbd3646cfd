"""What the label codecs of the two recognition heads (attn.AttnConvertor, ctc.CTCConvertor) share."""


def checked_beam_width(beam_width, limit):
    """A constructor's `beam_width` (None counts as 0: greedy decoding) as an int in 0..limit, the decoder's widest beam."""
    width = int(beam_width or 0)
    if not 0 <= width <= limit:
        raise ValueError(f"beam_width must lie in 0..{limit} (0: greedy decoding), got {beam_width}")
    return width


def nbest_lists(who, paths, lengths, scores, nbest):
    """A beam decoder's paths [N, W, T] (-1-padded), lengths [N, W] (-1: unused slot) and scores [N, W], by rank -> (indexes,
    log_probs): indexes[i] holds up to `nbest` index lists, best first (an unused slot gives none); log_probs is a float tensor
    [N, nbest] on the host.  `who` names the caller in the error."""
    nbest = int(nbest)
    if not 1 <= nbest <= paths.shape[1]:
        raise ValueError(f"{who}: nbest must lie in 1..beam_width = {paths.shape[1]}, got {nbest}")
    paths, lengths = paths[:, :nbest].cpu().numpy(), lengths[:, :nbest].cpu().numpy()
    indexes = [[paths[i, r, :lengths[i, r]].tolist() for r in range(nbest) if lengths[i, r] >= 0] for i in range(paths.shape[0])]
    return indexes, scores[:, :nbest].float().cpu()
