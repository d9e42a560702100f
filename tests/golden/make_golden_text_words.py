#!/usr/bin/env python3
"""Golden vectors for the word grouping of token-level timestamps from the REFERENCE's bundled tokenizer (build container only):
_combine_tokens_into_words and _collate_word_timestamps (tokenization_whisper.py) on the id sequences of text_timestamps.json plus
punctuation-heavy hand-made ones, over the toy byte-level BPE vocabulary of make_golden_text_timestamps.py.  Token k is given the
time span (0.06 k, 0.06 (k + 1)).  Output: tests/golden/text_words.json."""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/transformers/src"


def main():
    stub = types.ModuleType("transformers.dependency_versions_check")
    stub.dep_version_check = lambda *a, **k: None
    sys.modules["transformers.dependency_versions_check"] = stub
    sys.path.insert(0, REF_SRC)
    import transformers
    assert transformers.__version__ == "4.33.0.dev0" and transformers.__file__.startswith(REF_SRC)
    from transformers.models.whisper.tokenization_whisper import (WhisperTokenizer, _collate_word_timestamps,
                                                                  _combine_tokens_into_words)
    gold = json.load(open(os.path.join(HERE, "text_timestamps.json"), encoding="utf-8"))
    vocab, added, tb = gold["vocab"], gold["added_tokens"], gold["timestamp_begin"]
    merges = [("Ġ", "t"), ("h", "e"), ("Ġt", "he"), ("Ã", "©"), ("Ġ", "w"), ("o", "r"), ("Ġw", "or"), ("l", "d"), ("Ġwor", "ld")]
    tmp = tempfile.mkdtemp()
    json.dump(vocab, open(os.path.join(tmp, "vocab.json"), "w", encoding="utf-8"), ensure_ascii=False)
    open(os.path.join(tmp, "merges.txt"), "w", encoding="utf-8").write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    tok = WhisperTokenizer(os.path.join(tmp, "vocab.json"), os.path.join(tmp, "merges.txt"))
    tok.add_special_tokens({"additional_special_tokens": list(added)})
    assert {t: tok.convert_tokens_to_ids(t) for t in added} == added
    enc = lambda s: tok.encode(s, add_special_tokens=False)
    sot, eot = added["<|startoftranscript|>"], vocab["<|endoftext|>"]
    seqs = [c["ids"] for c in gold["cases"]] + [
        enc(" the world, the café!"),
        [sot] + enc(' "the world" (the) - world... the?!') + [eot],
        enc(" the [ world ] { the } : world ; the"),
        enc("the world's ¿the? ¡world! “the”"),
        enc(" wor-ld the.world , the 。world"),
        [sot, tb] + enc(" the") + [tb + 10] + enc(" ( world )") + [tb + 20, eot],
        enc(" é") [:-1] + enc(" the"),          # a cut multi-byte character: an invalid byte in the middle
        enc(" - the - world -"),
    ]
    out = {"text_timestamps": "vocab, added_tokens and timestamp_begin are those of text_timestamps.json", "cases": []}
    for ids in seqs:
        spans = [(round(0.06 * k, 2), round(0.06 * (k + 1), 2)) for k in range(len(ids))]
        words, word_tokens, indices = _combine_tokens_into_words(tok, list(ids), "english")
        timed = _collate_word_timestamps(tok, list(ids), spans, "english")
        out["cases"].append({"ids": list(ids), "spans": [list(s) for s in spans], "words": words, "word_tokens": word_tokens, "indices": indices,
                             "timed": [{"text": w["text"], "timestamp": list(w["timestamp"])} for w in timed]})
    json.dump(out, open(os.path.join(HERE, "text_words.json"), "w", encoding="utf-8"), ensure_ascii=False, indent=0)
    print("wrote text_words.json with", len(seqs), "cases; example:", out["cases"][7]["words"])


if __name__ == "__main__":
    main()
