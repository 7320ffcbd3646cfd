"""The decoding flags of test.py and train_finetune.py as the scripts declare them: both call ccd_amd.decoding_cli, so a test asks that
module for the parser instead of reading the scripts' text."""
import argparse
import os
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ("test.py", "train_finetune.py")


def declared(script):
    """(help text of every decoding flag of `script`, by flag; configure(argv) -> the config.decoder_* keys those arguments set)."""
    from ccd_amd import decoding_cli
    src = open(os.path.join(ROOT, script)).read()
    assert "decoding_cli.add_decoding_flags(" in src and "decoding_cli.apply_decoding_flags(" in src, script
    parser = argparse.ArgumentParser()
    decoding_cli.add_decoding_flags(parser, training="add_decoding_flags(parser, training=True)" in src)
    helps = {flag: action.help for action in parser._actions for flag in action.option_strings}

    def configure(argv):
        config = types.SimpleNamespace()
        decoding_cli.apply_decoding_flags(parser.parse_args(argv), config)
        return vars(config)
    return helps, configure
