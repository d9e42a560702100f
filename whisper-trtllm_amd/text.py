"""Text side of the evaluation loop: token ids -> text without `transformers`, and WER.

Reference: `hf_processor.batch_decode(predicted_ids, skip_special_tokens=True)` (examples/whisper/run.py:287) ==
WhisperTokenizer._decode / convert_tokens_to_string (transformers/models/whisper/tokenization_whisper.py:562-656), and
`jiwer.wer(references, hypotheses)` after a text normaliser (examples/whisper/cal_wer.py:279-287)."""
from __future__ import annotations

import json
import os
import re
import unicodedata
from typing import Dict, Iterable, List, Optional, Sequence


def _byte_decoder() -> Dict[str, int]:
    """Inverse of GPT-2's printable-byte alphabet: the 188 printable latin-1 bytes map to themselves, the other 68
    bytes to code points 256, 257, ... in increasing byte order."""
    printable = set(range(0x21, 0x7F)) | set(range(0xA1, 0xAD)) | set(range(0xAE, 0x100))
    table, nxt = {}, 256
    for b in range(256):
        if b in printable:
            table[chr(b)] = b
        else:
            table[chr(nxt)] = b
            nxt += 1
    return table


class WhisperTokenDecoder:
    """ids -> text for a byte-level BPE vocabulary (vocab.json: token string -> id)."""

    def __init__(self, vocab: Dict[str, int], added_tokens: Optional[Dict[str, int]] = None,
                 special_ids: Optional[Iterable[int]] = None, errors: str = "replace"):
        self.id_to_token = {i: t for t, i in vocab.items()}
        self.added = dict(added_tokens or {})
        for t, i in self.added.items():
            self.id_to_token[i] = t
        if special_ids is None:  # Whisper: <|endoftext|> and every added <|...|> token are special
            special_ids = [i for t, i in list(vocab.items()) + list(self.added.items()) if t.startswith("<|") and t.endswith("|>")]
        self.special_ids = set(special_ids)
        # timestamp tokens <|t|> sit above every special id (the reference's all_special_ids[-1] + 1, tokenization_whisper.py:504)
        self.timestamp_begin = max(self.special_ids) + 1 if self.special_ids else max(self.id_to_token, default=-1) + 1
        self.byte_decoder = _byte_decoder()
        self.errors = errors

    @classmethod
    def from_dir(cls, path: str) -> "WhisperTokenDecoder":
        vocab = json.load(open(os.path.join(path, "vocab.json"), encoding="utf-8"))
        added_path = os.path.join(path, "added_tokens.json")
        added = json.load(open(added_path, encoding="utf-8")) if os.path.exists(added_path) else {}
        return cls(vocab, added)

    def _bytes_to_text(self, tokens: List[str]) -> str:
        return bytearray(self.byte_decoder[c] for c in "".join(tokens)).decode("utf-8", errors=self.errors)

    def _strip_prompt(self, ids: Sequence[int]) -> List[int]:
        """The reference tokenizer's _strip_prompt (tokenization_whisper.py): ids that begin with <|startofprev|> lose everything in
        front of <|startoftranscript|> (all of them when there is none); other ids are returned as they are."""
        ids = [int(i) for i in ids]
        prev, sot = self.added.get("<|startofprev|>"), self.added.get("<|startoftranscript|>")
        if prev is None or not ids or ids[0] != prev:
            return ids
        return ids[ids.index(sot):] if sot in ids else []

    def decode(self, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
        """skip_special_tokens also drops a leading decoder prompt (<|startofprev|> ... up to the start token), as the reference does."""
        parts, run = [], []
        if skip_special_tokens:
            ids = self._strip_prompt(ids)
        for i in ids:
            i = int(i)
            if (skip_special_tokens and i in self.special_ids) or i >= self.timestamp_begin:   # timestamps decode to nothing
                continue
            tok = self.id_to_token[i]
            if tok in self.added:          # added tokens are literal text, not byte-level symbols
                if run:
                    parts.append(self._bytes_to_text(run))
                    run = []
                parts.append(tok)
            else:
                run.append(tok)
        if run:
            parts.append(self._bytes_to_text(run))
        return "".join(parts)

    def decode_with_timestamps(self, ids: Sequence[int], skip_special_tokens: bool = False, time_precision: float = 0.02) -> str:
        """Text with every timestamp token written as "<|1.08|>" (the reference's _decode_with_timestamps, tokenization_whisper.py:499-518)."""
        outputs: List = [[]]
        for i in ids:
            i = int(i)
            if i >= self.timestamp_begin:
                outputs.append(f"<|{(i - self.timestamp_begin) * time_precision:.2f}|>")
                outputs.append([])
            else:
                outputs[-1].append(i)
        return "".join(o if isinstance(o, str) else self.decode(o, skip_special_tokens) for o in outputs)

    def offsets(self, ids: Sequence[int], time_precision: float = 0.02) -> List[dict]:
        """Segments [{"text", "timestamp": (start s, end s)}] between timestamp pairs (the reference's _compute_offsets,
        tokenization_whisper.py:520-560): a segment runs from one timestamp to the next pair of consecutive timestamps (or to the
        last timestamp); text keeps the special tokens."""
        ids = [int(i) for i in ids]
        is_ts = [i >= self.timestamp_begin for i in ids]
        where = [k for k, t in enumerate(is_ts) if t]
        cuts = [k + 1 for k in range(len(ids) - 1) if is_ts[k] and is_ts[k + 1]]
        if not cuts and len(where) <= 1:
            return []
        if where[-1] + 1 not in cuts:
            cuts.append(where[-1] + 1)
        out, last = [], where[0]
        for cur in cuts:
            piece = ids[last:cur]
            if len(piece) > 1:
                out.append({"text": self.decode(piece, skip_special_tokens=False),
                            "timestamp": ((piece[0] - self.timestamp_begin) * time_precision, (piece[-1] - self.timestamp_begin) * time_precision)})
            last = cur
        return out

    # ---- word grouping for token-level timestamps (the reference's _combine_tokens_into_words and helpers,
    # tokenization_whisper.py:1087-1215), space-separated languages
    def _split_on_unicode(self, ids: List[int]):
        """Cut wherever the tokens so far decode to complete unicode code points (_split_tokens_on_unicode)."""
        full = self.decode_with_timestamps(ids)
        bad = "\ufffd"
        words, word_tokens, indices, cur, cur_idx, offset = [], [], [], [], [], 0
        for k, tok in enumerate(ids):
            cur.append(tok)
            cur_idx.append(k)
            text = self.decode_with_timestamps(cur)
            if bad not in text or full[offset + text.index(bad)] == bad:
                words.append(text)
                word_tokens.append(cur)
                indices.append(cur_idx)
                cur, cur_idx = [], []
                offset += len(text)
        return words, word_tokens, indices

    def _split_on_spaces(self, ids: List[int]):
        """Join the unicode pieces into words at leading spaces, punctuation and special tokens (_split_tokens_on_spaces)."""
        eos = self.eos_token_id
        words, word_tokens, indices = [], [], []
        for sub, toks, idx in zip(*self._split_on_unicode(ids)):
            special = toks[0] >= eos
            punctuation = sub.strip() in "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
            if special or sub.startswith(" ") or punctuation or not words:
                words.append(sub)
                word_tokens.append(list(toks))
                indices.append(list(idx))
            else:
                words[-1] += sub
                word_tokens[-1].extend(toks)
                indices[-1].extend(idx)
        return words, word_tokens, indices

    @staticmethod
    def _merge_punctuations(words, tokens, indices, prepended, appended):
        i, j = len(words) - 2, len(words) - 1
        while i >= 0:       # opening punctuation joins the word after it
            if words[i].startswith(" ") and words[i].strip() in prepended:
                words[j], tokens[j], indices[j] = words[i] + words[j], tokens[i] + tokens[j], indices[i] + indices[j]
                words[i], tokens[i], indices[i] = "", [], []
            else:
                j = i
            i -= 1
        i, j = 0, 1
        while j < len(words):   # closing punctuation joins the word before it
            if not words[i].endswith(" ") and words[j] in appended:
                words[i] += words[j]
                tokens[i] += tokens[j]
                indices[i] += indices[j]
                words[j], tokens[j], indices[j] = "", [], []
            else:
                i = j
            j += 1
        words[:] = [w for w in words if w]
        tokens[:] = [t for t in tokens if t]
        indices[:] = [x for x in indices if x]

    @property
    def eos_token_id(self) -> int:
        eot = [i for i, t in self.id_to_token.items() if t == "<|endoftext|>"]
        if not eot:
            raise ValueError("the vocabulary has no <|endoftext|> token")
        return eot[0]

    def combine_tokens_into_words(self, ids: Sequence[int], prepend_punctuations: str = "\"'\u201c\u00a1\u00bf([{-",
                                  append_punctuations: str = "\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001"):
        """(words, token ids per word, token positions per word) of a space-separated language (_combine_tokens_into_words)."""
        words, word_tokens, indices = self._split_on_spaces([int(i) for i in ids])
        self._merge_punctuations(words, word_tokens, indices, prepend_punctuations, append_punctuations)
        return words, word_tokens, indices

    def words(self, ids: Sequence[int], token_timestamps: Sequence) -> List[dict]:
        """[{"text", "timestamp": (start s, end s)}] per word (_collate_word_timestamps).  `token_timestamps` holds one entry per id:
        either (start, end) pairs, or the start times `generate(..., return_token_timestamps=True)` returns -- a token then ends where
        the next one starts, the last one where it starts.  Space-separated languages only."""
        ids = [int(i) for i in ids]
        ts = list(token_timestamps)
        if len(ts) != len(ids):
            raise ValueError(f"{len(ids)} ids but {len(ts)} token timestamps")
        if ts and not isinstance(ts[0], (tuple, list)):
            ts = [float(t) for t in ts]
            ts = [(ts[k], ts[k + 1] if k + 1 < len(ts) else ts[k]) for k in range(len(ts))]
        words, _tok, indices = self.combine_tokens_into_words(ids)
        return [{"text": w, "timestamp": (ts[idx[0]][0], ts[idx[-1]][1])} for w, idx in zip(words, indices)]

    def batch_decode(self, batch: Iterable[Sequence[int]], skip_special_tokens: bool = True) -> List[str]:
        return [self.decode(ids, skip_special_tokens) for ids in batch]


def compression_ratio(text: str) -> float:
    """openai-whisper's compression ratio of a transcript: len(utf-8 bytes) / len(zlib.compress(utf-8 bytes)).  Repetitive
    (hallucinated) text compresses well; whisper's fallback loop rejects a segment above 2.4."""
    import zlib
    data = text.encode("utf-8")
    return len(data) / len(zlib.compress(data))


def basic_normalize(text: str) -> str:
    """Lower-case, drop bracketed/parenthesised spans, turn symbols and punctuation into spaces, collapse whitespace
    (the behaviour of the bundled BasicTextNormalizer, english_normalizer.py:75-91, plus a final strip; the full English
    normaliser with contraction, number and spelling rules is `whisper_trtllm_amd.english.EnglishTextNormalizer`)."""
    s = text.lower()
    s = re.sub(r"[<\[][^>\]]*[>\]]", "", s)
    s = re.sub(r"\(([^)]+?)\)", "", s)
    s = "".join(" " if unicodedata.category(c)[0] in "MSP" else c for c in unicodedata.normalize("NFKC", s))
    return re.sub(r"\s+", " ", s).strip()


def _edit_distance(ref: Sequence[str], hyp: Sequence[str]) -> int:
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i] + [0] * len(hyp)
        for j, h in enumerate(hyp, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r != h))
        prev = cur
    return prev[-1]


def word_error_rate(references: Sequence[str], hypotheses: Sequence[str]) -> float:
    """(substitutions + deletions + insertions) / reference words, pooled over all utterances (jiwer.wer semantics)."""
    if len(references) != len(hypotheses):
        raise ValueError("references and hypotheses differ in length")
    errors = words = 0
    for r, h in zip(references, hypotheses):
        rw, hw = r.split(), h.split()
        errors += _edit_distance(rw, hw)
        words += len(rw)
    if words == 0:
        raise ValueError("no reference words")
    return errors / words
