#!/usr/bin/env python3
"""Golden vectors for timestamp-token decoding from the REFERENCE's bundled WhisperTokenizer (build container only).
The toy byte-level BPE vocabulary of make_golden_text.py; ids at and above timestamp_begin (= the last special id + 1, as the reference
computes it) are timestamp tokens.  Per case: decode (keep / skip special tokens), decode_with_timestamps=True and output_offsets=True.
Output: tests/golden/text_timestamps.json."""
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
    from transformers.models.whisper.tokenization_whisper import WhisperTokenizer, bytes_to_unicode

    b2u = bytes_to_unicode()
    symbols = [b2u[b] for b in range(256)]
    merges = [("Ġ", "t"), ("h", "e"), ("Ġt", "he"), ("Ã", "©"), ("Ġ", "w"), ("o", "r"), ("Ġw", "or"), ("l", "d"), ("Ġwor", "ld")]
    vocab = {s: i for i, s in enumerate(symbols)}
    for a, b in merges:
        vocab[a + b] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    tmp = tempfile.mkdtemp()
    json.dump(vocab, open(os.path.join(tmp, "vocab.json"), "w", encoding="utf-8"), ensure_ascii=False)
    open(os.path.join(tmp, "merges.txt"), "w", encoding="utf-8").write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    tok = WhisperTokenizer(os.path.join(tmp, "vocab.json"), os.path.join(tmp, "merges.txt"))
    extra = ["<|startoftranscript|>", "<|startofprev|>", "<|notimestamps|>"]
    tok.add_special_tokens({"additional_special_tokens": extra})
    added = {t: tok.convert_tokens_to_ids(t) for t in extra}
    tb = tok.all_special_ids[-1] + 1
    assert tb == max(added.values()) + 1
    eot, sot = vocab["<|endoftext|>"], added["<|startoftranscript|>"]
    the, world = tok.encode(" the", add_special_tokens=False), tok.encode(" world", add_special_tokens=False)
    cafe = tok.encode(" café!", add_special_tokens=False)
    seqs = [
        [sot] + the + world + [eot],                                                     # no timestamps
        [sot, tb] + the + world + [eot],                                                 # a single timestamp
        [sot, tb] + the + [tb + 50, tb + 50] + world + [tb + 101, eot],                  # pairs, last one unpaired before EOS
        [sot, tb + 3] + the + [tb + 40, tb + 41] + cafe + [tb + 90, tb + 91] + world + [tb + 120],   # trailing unpaired timestamp
        [tb + 7, tb + 9] + world,                                                        # consecutive first, text last
        [sot, tb, tb + 1500] + cafe + [eot],                                             # the last timestamp (30.00 s)
    ]
    out = {"vocab": vocab, "added_tokens": added, "timestamp_begin": tb, "cases": []}
    for ids in seqs:
        off = tok.decode(ids, output_offsets=True)["offsets"]
        out["cases"].append({"ids": ids, "keep": tok.decode(ids, skip_special_tokens=False), "skip": tok.decode(ids, skip_special_tokens=True),
                             "with_timestamps": tok.decode(ids, decode_with_timestamps=True),
                             "offsets": [{"text": o["text"], "timestamp": list(o["timestamp"])} for o in off]})
    json.dump(out, open(os.path.join(HERE, "text_timestamps.json"), "w", encoding="utf-8"), ensure_ascii=False, indent=0)
    print("wrote text_timestamps.json with", len(seqs), "cases; example:", repr(out["cases"][2]["with_timestamps"]), out["cases"][2]["offsets"])


if __name__ == "__main__":
    main()
