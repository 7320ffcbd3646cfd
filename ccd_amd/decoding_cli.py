"""The decoding flags of test.py and train_finetune.py, declared once: --beam_width, --lexicon, --lexicon_beam, the --lm group,
--joint_ctc_weight and --twopass_beam / --twopass_ctc_weight, their copy into `config.decoder_*`, and the log lines that say which lexicon and language model the built model
decodes with."""
from __future__ import annotations

import logging

DECODING_FLAGS = ("beam_width", "lexicon", "lexicon_beam", "lm", "lm_weight", "lm_bonus", "joint_ctc_weight", "twopass_beam",
                  "twopass_ctc_weight")      # flag `--x` sets `config.decoder_x`


def add_decoding_flags(parser, training=False):
    """training: the flags of train_finetune.py, where they configure the evaluation rounds and two help texts say so."""
    parser.add_argument("--beam_width", type=int, default=None,
                        help=("evaluate with beam search of this width, 1..16, for either head (CTC: prefix beam search; NRTR: beam over the decoder); 0: greedy"
                              if training else
                              "beam search of this width, 1..16, for either head (CTC: prefix beam search; NRTR: beam over the decoder); 0: greedy decoding"))
    parser.add_argument("--lexicon", type=str, default=None,
                        help="evaluate with lexicon-constrained decoding over this UTF-8 word list (one word per line); excludes a beam.  The NRTR "
                             "head needs --lexicon_beam with it")
    parser.add_argument("--lexicon_beam", type=int, default=None,
                        help="with a lexicon: search its prefix tree with a beam of this width, 1..16, and score only the proposed words "
                             "exactly - the cost no longer grows with the lexicon; 0: score every word (CTC head).  NRTR head: the width of the "
                             "beam over the decoder that walks the lexicon's prefix tree, 1..16; its scores are exact already")
    parser.add_argument("--lm", type=str, default=None,
                        help=("evaluate the CTC head with a character n-gram language model fused into the beam search" if training else
                              "fuse a character n-gram language model into the CTC beam search") +
                        ": an .npz of CharNGram.save, or a UTF-8 word list (estimated at decoder.lm_order); needs a beam, excludes a lexicon")
    parser.add_argument("--lm_weight", type=float, default=None, help="weight of the language model's log-probabilities (default 1.0)")
    parser.add_argument("--lm_bonus", type=float, default=None, help="added per decoded character (default 0.0)")
    parser.add_argument("--joint_ctc_weight", type=float, default=None,
                        help="NRTR head with an auxiliary CTC head (decoder.aux_ctc_weight): joint CTC / attention decoding - the beam over the "
                             "decoder is rescored with the CTC prefix probability of every candidate at this weight, 0..1; needs --beam_width "
                             "1..16, excludes a lexicon")
    parser.add_argument("--twopass_beam", type=int, default=None,
                        help="NRTR head with an auxiliary CTC head (decoder.aux_ctc_weight): two-pass decoding - the CTC prefix beam of this "
                             "width, 1..16, proposes words, the NRTR decoder scores all of them in one teacher-forced pass and the two exact "
                             "scores rank them again; excludes --beam_width, a lexicon and --joint_ctc_weight")
    parser.add_argument("--twopass_ctc_weight", type=float, default=None,
                        help="with --twopass_beam: the weight of the CTC score in (1 - w) attention + w CTC, 0..1 (default 0.5, untuned)")


def apply_decoding_flags(args, config):
    """Every decoding flag that was given replaces its `config.decoder_*` key (config.decoder_beam_width = args.beam_width, ...)."""
    for key in DECODING_FLAGS:
        if getattr(args, key) is not None:
            setattr(config, f"decoder_{key}", getattr(args, key))


def log_decoding(convertor, config):
    if getattr(convertor, "twopass_beam", 0):
        logging.info(f"two-pass decoding: the CTC beam of width {convertor.twopass_beam} proposes, the NRTR decoder rescores at "
                     f"twopass_ctc_weight {convertor.twopass_ctc_weight}")
    if getattr(convertor, "lexicon_stats", None):
        logging.info(f"lexicon {config.decoder_lexicon} (lexicon_beam {getattr(convertor, 'lexicon_beam', 0)}): {convertor.lexicon_stats}")
    if getattr(convertor, "lm_stats", None):
        logging.info(f"language model {config.decoder_lm}: {convertor.lm_stats}, weight {convertor.lm_weight}, bonus {convertor.lm_bonus}, "
                     f"eos {convertor.lm_eos}")
