#!/usr/bin/env python3
"""Benchmark evaluation of a finetuned recogniser on MI355X - the reference's test.py (CLI :30-90, loop :156-218):

    python test.py --config Dino/configs/CCD_vision_model_ARD.yaml        # model.checkpoint = a {net, ...} file

Builds DINO_Finetune(config), loads `checkpoint['net']` (DataParallel-prefixed keys, as train_finetune.py and the
published ARD / STD files store them), evaluates every entry of `dataset.test.roots` with TextAccuracy and prints the
reference's report: one line per dataset (word_num, accuracy = cwr) and the word-weighted total.
"""
import argparse
import json
import logging
import os

import torch
import torch.utils.data

from Dino.metric.eval_acc import TextAccuracy
from Dino.model.dino_vision import DINO_Finetune
from Dino.modules import utils
from Dino.utils.utils import Config, Logger
from ccd_amd import decoding_cli
from ccd_amd.dataset.dataset_pretrain import ImageDataset, collate_fn_filter_none
from ccd_amd.parallel import DataParallel
from train import _lmdb_dirs

EVAL_DATA_NAMES = ["IIIT5k_3000", "SVT", "IC13_1015", "IC15_1811", "SVTP", "CUTE80", "TotalText", "COCOText", "CTW", "HOST",
                   "WOST"]                                        # test.py:184-196 (the order of dataset.test.roots)


def get_test_loaders(config):
    """One loader per entry of dataset.test.roots; an entry with sub-folders is the concatenation of its LMDBs (test.py:111-121)."""
    kw = dict(img_h=int(config.dataset_image_height or 32), img_w=int(config.dataset_image_width or 128),
              max_length=int(config.decoder_max_seq_len or 25), type=config.dataset_charset_type or "DICT90", is_training=False)
    loaders = []
    for eval_root in config.dataset_test_roots:
        parts = [ImageDataset(path=p, **kw) for p in _lmdb_dirs([eval_root])]
        ds = parts[0] if len(parts) == 1 else torch.utils.data.ConcatDataset(parts)
        loaders.append(torch.utils.data.DataLoader(ds, batch_size=int(config.dataset_test_batch_size or 256), shuffle=False,
                                                   num_workers=int(config.dataset_num_workers or 0),
                                                   collate_fn=collate_fn_filter_none, pin_memory=bool(config.dataset_pin_memory),
                                                   drop_last=False))
    return loaders


def alignment_writer(convertor, out, name, image_width=128):
    """The per-batch hook of --alignments: one JSON line per image - ground truth, the predicted word (what the convertor's
    configuration decodes: greedy, beam, LM-fused beam or lexicon), the log-probability of its best alignment and its characters with
    x0, x1 (pixels of the crop), first and last frame and conf.  A character's span is where the network EMITS it, not its inked
    extent.  One device-to-host copy per batch (CTCConvertor.tensor2chars); `pred` is null where the decoder returned no word that
    can be aligned."""
    count = [0]

    def write(probs, gts):
        for gt, entries in zip(gts, convertor.tensor2chars(probs, nbest=1, normalized=True, image_width=image_width)):
            word, log_prob, chars = entries[0] if entries else (None, None, [])
            out.write(json.dumps({"dataset": name, "index": count[0], "gt": gt, "pred": word, "log_prob": log_prob,
                                  "chars": [dict(zip(("char", "x0", "x1", "first", "last", "conf"), c)) for c in chars]},
                                 ensure_ascii=False) + "\n")
            count[0] += 1
    return write


def decoded_words(net, images):
    """The word the NRTR head's configured decoder returns for every image, as class indices (None: the lexicon's beam ended without
    a word): rank 0 of forward_twopass (twopass_beam), of forward_lexicon (a lexicon and its lexicon_beam), of forward_beam at
    beam_width, or of the beam of width 1, which is greedy decoding."""
    conv = net.label_convertor
    if getattr(conv, "twopass_beam", 0) > 0:
        paths, lengths, _ = net.forward_twopass(images)
    elif conv.lexicon is not None:
        _, _, paths, lengths = net.forward_lexicon(images)
    else:
        paths, lengths, _ = net.forward_beam(images, conv.beam_width if conv.beam_width > 0 else 1)
    paths, lengths = paths[:, 0].cpu().numpy(), lengths[:, 0].cpu().numpy()
    return [None if n < 0 else paths[i, :n].tolist() for i, n in enumerate(lengths.tolist())]


def write_char_scores(model, loaders, config, out, names=None):
    """--char_scores: a pass of its own over the test sets, behind the accuracy run and changing nothing of it - one JSON line per image:
    ground truth, the word the configured decoder returns (`decoded_words`), its log-probability log p(word <EOS> | image), and per
    character conf = p(character | the ones before it) with the centre and box of the decoder's attention in pixels of the crop, all
    from ONE DINO_Finetune.forward_score pass per batch (AttnConvertor.scores2chars).  A box is where the decoder LOOKS when it writes
    the character, not the extent of the ink.  `pred` is null where the decoder returned no word."""
    names = names or EVAL_DATA_NAMES
    net = model.module if hasattr(model, "module") else model
    net.eval()
    conv = net.label_convertor
    device = next(net.parameters()).device
    hw = (int(config.dataset_image_height or 32), int(config.dataset_image_width or 128))
    with torch.no_grad():
        for i, loader in enumerate(loaders):
            name, count = names[i] if i < len(names) else f"dataset{i}", 0
            for image_tensors, label_tensors in loader:
                image_tensors = image_tensors.to(device)
                words = [[w] if w is not None else [] for w in decoded_words(net, image_tensors)]
                seq, row_ptr, _ = conv.words2rows(words)
                records = conv.scores2chars(net.forward_score(image_tensors, words), seq, img_hw=hw)
                for b, gt in enumerate(list(label_tensors[0])):
                    rec = records[int(row_ptr[b])] if words[b] else {"word": None, "log_prob": None, "eos_conf": None, "chars": []}
                    out.write(json.dumps({"dataset": name, "index": count, "gt": gt, "pred": rec["word"], "log_prob": rec["log_prob"],
                                          "eos_conf": rec["eos_conf"], "chars": rec["chars"]}, ensure_ascii=False) + "\n")
                    count += 1


def evaluate(model, loaders, config, names=None, alignments=None):
    """alignments: a text file open for writing (--alignments); None: nothing but the accuracy run."""
    names = names or EVAL_DATA_NAMES
    words = acc = 0.0
    report, results = "", []
    model.eval() if not hasattr(model, "module") else model.module.eval()
    with torch.no_grad():
        for i, loader in enumerate(loaders):
            metric = TextAccuracy(charset_path=config.dataset_charset_path, case_sensitive=bool(config.dataset_eval_case_sensitive),
                                  model_eval="vision")
            name = names[i] if i < len(names) else f"dataset{i}"
            if alignments is None:
                res = metric.compute(model, loader)
            else:
                net = model.module if hasattr(model, "module") else model
                res = metric.compute(model, loader, on_batch=alignment_writer(
                    net.label_convertor, alignments, name, image_width=int(config.dataset_image_width or 128)))
            results.append(res)
            acc += res["cwr"] * res["words"]
            words += res["words"]
            report += f"dataset: {name} --> word_num: {res['words']} --> accuracy: {res['cwr']:0.3f}\n"
    report += f"total_accuracy: {acc / max(words, 1.0):0.3f}"
    return report, results


def check_arguments(a):
    """What can be refused before anything is built."""
    if a.char_scores is not None and a.alignments is not None:
        raise ValueError("--char_scores (the NRTR head) and --alignments (the CTC head) exclude each other: a model has one head")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="Dino/configs/CCD_vision_model_ARD.yaml", help="path to config file")
    ap.add_argument("--checkpoint", type=str, default=None)
    ap.add_argument("--test_root", type=str, default=None)
    ap.add_argument("--batch_size", type=int, default=None)
    decoding_cli.add_decoding_flags(ap)
    ap.add_argument("--alignments", type=str, default=None, metavar="PATH",
                    help="next to the accuracy run write one JSON line per image to PATH - ground truth, predicted word, the log-probability of "
                         "its best alignment, and per character x0, x1, first / last frame and confidence (the CTC head only)")
    ap.add_argument("--char_scores", type=str, default=None, metavar="PATH",
                    help="behind the accuracy run write one JSON line per image to PATH - ground truth, the word the configured decoder returns "
                         "(greedy, --beam_width, or --lexicon with --lexicon_beam), its log-probability, and per character the confidence and "
                         "the box of the decoder's attention (the NRTR head only; the CTC head has --alignments)")
    a = ap.parse_args()
    check_arguments(a)
    config = Config(a.config)
    if a.checkpoint is not None:
        config.model_checkpoint = a.checkpoint
    if a.test_root is not None:
        config.dataset_test_roots = [a.test_root]
    if a.batch_size is not None:
        config.dataset_test_batch_size = a.batch_size
    decoding_cli.apply_decoding_flags(a, config)
    Logger.init(config.global_workdir, config.global_name, "test")
    utils.fix_random_seeds(int(config.global_seed or 0))
    logging.info("Construct dataset.")
    loaders = get_test_loaders(config)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    model = DINO_Finetune(config).to(device)
    decoding_cli.log_decoding(model.label_convertor, config)
    model.ensure_arena()
    model = DataParallel(model)
    if config.model_checkpoint:
        logging.info(f"Read vision model from {config.model_checkpoint}.")
        sd = torch.load(config.model_checkpoint, map_location="cpu", weights_only=False)
        model.load_state_dict(sd["net"])
        model.module.ensure_arena()
    logging.info("eval model")
    if a.char_scores is not None and model.module.ctc:
        raise NotImplementedError("--char_scores is for the NRTR head only: the CTC head writes character spans and confidences with "
                                  "--alignments")
    if (a.char_scores is not None or a.alignments is not None) and model.module.par:
        raise NotImplementedError("--char_scores (the NRTR head) and --alignments (the CTC head) are not for the parallel attention head: "
                                  "its attention maps are DINO_Finetune.forward_attn's")
    if a.alignments is not None:
        if not model.module.ctc:
            raise NotImplementedError("--alignments is for the CTC head only: the NRTR decoder has no frame axis to align a word against")
        with open(a.alignments, "w", encoding="utf-8") as f:
            report, _ = evaluate(model, loaders, config, alignments=f)
    else:
        report, _ = evaluate(model, loaders, config)
    if a.char_scores is not None:
        with open(a.char_scores, "w", encoding="utf-8") as f:
            write_char_scores(model, loaders, config, f)
    print("-" * 80)
    print(report + "\n")


if __name__ == "__main__":
    main()
