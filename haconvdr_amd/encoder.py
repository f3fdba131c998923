"""Encoder seam of the reference, host-side mirror.

``ANCEEncoder`` is called exactly like the reference's module: ``model(input_ids,
attention_mask)`` with integer tensors [B, L] (src/test_HAConvDR_topiocqa.py:211,
gen_doc_embeddings.py:110) and returns a float32 tensor [B, 768] on the same device
(= src/models.py:44).  Weights use the checkpoint's own key names (``roberta.*``,
``embeddingHead.*``, ``norm.*``; ``classifier.*`` is ignored as in the reference's forward).
``BERTEncoder`` is the same seam for the reference's ``BERT`` class (src/models.py:66-110, load_model's BERT_* types):
``bert.*`` names, position ids arange(L), the same kernels behind the embedding stage.
All arithmetic runs in the gfx950 HIP kernels of libhaconvdr.so; there is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib


def split_bf16(x):
    """Host twin of the kernels' split_bf16 (csrc/split.inc): the pair (hi, lo) = (bf16(x), bf16(x - float(hi))) of a float32
    array, both returned as float32.  hi + lo reproduces x to 2^-16 relative (round to nearest even twice: 2^-9 of 2^-9 is the
    bound, 2^-17 the typical figure) wherever lo is a normal bf16 value, and is never worse than hi alone."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy(), lo.numpy()


class ANCEEncoder:
    MODEL = "roberta"            # the "model" option of the handle (include/haconvdr.h): tensor names, position rule, length bound
    KEY_PREFIX = "roberta."      # the checkpoint's name prefix of the transformer's tensors
    UNUSED_PREFIXES = ("classifier.",)          # present in the checkpoint, unused by forward (models.py:26)
    CONFIG_DEFAULTS = {"ln_eps": 1e-5, "pad_token_id": 1}    # RobertaConfig's, where config.json is silent

    def __init__(self, n_layers=12, vocab=50265, max_pos=514, type_vocab=1, pad_token_id=1, ln_eps=1e-5, device=0, precision="bf16",
                 pooling="first"):
        self.device = int(device)
        self.n_layers = int(n_layers)
        cfg = _lib.EncoderConfig(self.n_layers, 768, 12, 3072, int(vocab), int(max_pos), int(type_vocab), int(pad_token_id), float(ln_eps))
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().hac_encoder_create(ctypes.byref(cfg), self.device, ctypes.byref(self._h)))
        if self.MODEL != "roberta":  # before the first tensor: the names hac_encoder_finalize asks for follow it
            self.set_option("model", self.MODEL)
        if precision != "bf16":     # "split": hi + lo bf16 operand pairs, three MFMAs per product (include/haconvdr.h, "precision")
            self.set_option("precision", precision)
        self._pooling = "first"
        if pooling != "first":      # "mean": the reference's use_mean = True (src/models.py:52-61), see the use_mean property
            self.set_option("pooling", pooling)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().hac_encoder_destroy(h)
            except Exception:
                pass

    # ---- weights -----------------------------------------------------------
    def load_state_dict(self, sd):
        """sd: name -> float32 array / torch tensor with the reference checkpoint's names."""
        L = _lib.lib()
        for name, v in sd.items():
            if name.startswith(self.UNUSED_PREFIXES) or name.endswith("position_ids"):
                continue                       # present in the checkpoint, unused by forward (models.py:26, :72)
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            _lib.check(L.hac_encoder_set_weight(self._h, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size))
        _lib.check(L.hac_encoder_finalize(self._h))
        return self

    @classmethod
    def from_state_dict(cls, sd, device=0, **kw):
        p = cls.KEY_PREFIX
        n_layers = cls._count_layers(sd)
        vocab, _ = np.shape(sd[p + "embeddings.word_embeddings.weight"])
        max_pos, _ = np.shape(sd[p + "embeddings.position_embeddings.weight"])
        tv, _ = np.shape(sd[p + "embeddings.token_type_embeddings.weight"])
        return cls(n_layers=n_layers, vocab=vocab, max_pos=max_pos, type_vocab=tv, device=device, **kw).load_state_dict(sd)

    @classmethod
    def _count_layers(cls, sd):
        layers = [int(k.split(".")[3]) for k in sd if k.startswith(cls.KEY_PREFIX + "encoder.layer.")]
        if not layers or cls.KEY_PREFIX + "embeddings.word_embeddings.weight" not in sd:
            raise ValueError(f"no {cls.KEY_PREFIX}* tensors in the state dict: not a checkpoint {cls.__name__} reads")
        return 1 + max(layers)

    @classmethod
    def from_pretrained(cls, path, device=0, precision="bf16", pooling="first"):
        """Checkpoint directory as ``ANCE.from_pretrained(model_path, config=RobertaConfig.from_pretrained(model_path))``
        reads it (src/models.py:113-122): ``config.json`` + ``pytorch_model.bin`` or ``model.safetensors``.

        config.json supplies what the tensors cannot: ``layer_norm_eps`` and ``pad_token_id`` (position ids), and is
        checked against them — layer count, hidden / FFN / head geometry, vocabulary, positions, activation.  A
        checkpoint this encoder was not built for is refused here, not mis-encoded."""
        import json
        import os
        import torch
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
        sd = {k: v.float() for k, v in sd.items()}
        kw = {}
        cfg_path = os.path.join(path, "config.json")
        if os.path.exists(cfg_path):
            with open(cfg_path) as f:
                cfg = json.load(f)
            if cls.MODEL != "roberta" and cfg.get("model_type", cls.MODEL) != cls.MODEL:
                raise ValueError(f"{cfg_path}: model_type = {cfg['model_type']!r}; {cls.__name__} reads {cls.MODEL!r} checkpoints")
            p = cls.KEY_PREFIX
            n_layers = cls._count_layers(sd)
            vocab, hidden = sd[p + "embeddings.word_embeddings.weight"].shape
            found = {"num_hidden_layers": n_layers, "hidden_size": hidden, "vocab_size": vocab,
                     "max_position_embeddings": sd[p + "embeddings.position_embeddings.weight"].shape[0],
                     "type_vocab_size": sd[p + "embeddings.token_type_embeddings.weight"].shape[0],
                     "intermediate_size": sd[p + "encoder.layer.0.intermediate.dense.weight"].shape[0]}
            for key, have in found.items():
                if key in cfg and int(cfg[key]) != int(have):
                    raise ValueError(f"{cfg_path}: {key} = {cfg[key]} but the checkpoint's tensors say {have}")
            if int(cfg.get("num_attention_heads", 12)) != 12 or int(cfg.get("hidden_size", 768)) != 768 or int(cfg.get("intermediate_size", 3072)) != 3072:
                raise ValueError(f"{cfg_path}: only the base geometry is built (hidden 768, 12 heads, FFN 3072)")
            if cfg.get("hidden_act", "gelu") != "gelu":
                raise ValueError(f"{cfg_path}: hidden_act = {cfg['hidden_act']!r}; the kernels implement erf GELU")
            if cfg.get("position_embedding_type", "absolute") != "absolute":
                raise ValueError(f"{cfg_path}: position_embedding_type = {cfg['position_embedding_type']!r} is not supported")
            pad = cfg.get("pad_token_id")   # (may be null in a hand-written config)
            kw = {"ln_eps": float(cfg.get("layer_norm_eps", cls.CONFIG_DEFAULTS["ln_eps"])),
                  "pad_token_id": int(cls.CONFIG_DEFAULTS["pad_token_id"] if pad is None else pad)}
        return cls.from_state_dict(sd, device=device, precision=precision, pooling=pooling, **kw)

    # ---- forward -----------------------------------------------------------
    def __call__(self, input_ids, attention_mask, wrap_pooler=False):
        """model(input_ids, attention_mask) -> float32 [B, 768].  torch CUDA tensors stay on the GPU
        (enqueued on the current stream); numpy / CPU inputs take the synchronous host path."""
        import torch
        if isinstance(input_ids, torch.Tensor) and input_ids.is_cuda:
            ids = input_ids.contiguous()
            mask = attention_mask.to(ids.dtype).contiguous()
            if ids.dtype not in (torch.int32, torch.int64):
                ids, mask = ids.long(), mask.long()
            B, L = ids.shape
            out = torch.empty((B, 768), dtype=torch.float32, device=ids.device)
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().hac_encoder_forward_device(self._h, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(mask.data_ptr()),
                                                            ids.element_size(), B, L, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st)))
            return out
        ids = np.ascontiguousarray(np.asarray(input_ids), dtype=np.int32)
        mask = np.ascontiguousarray(np.asarray(attention_mask), dtype=np.int32)
        B, L = ids.shape
        out = np.empty((B, 768), np.float32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        _lib.check(_lib.lib().hac_encoder_forward(self._h, ids.ctypes.data_as(i32p), mask.ctypes.data_as(i32p), B, L,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return torch.from_numpy(out) if isinstance(input_ids, torch.Tensor) else out

    forward = query_emb = doc_emb = __call__       # models.py:39-49,63-64

    def layer_state(self, input_ids, attention_mask, layer, normalized=False):
        """Test aid (hac_encoder_layer_state): the residual stream after encoder layer ``layer`` (-1: the embedding LayerNorm,
        at most n_layers - 2; with pooling = "mean" the last layer too, n_layers - 1), from the same kernels a forward of this batch runs.  Returns a dict of numpy arrays over
        [B, L] (rows t >= len are zeros): ``rows`` float32 [B, L, 768], the pre-LayerNorm rows as stored (fp32 on the classic
        path, bf16 values on gemm8); ``mean``, ``rstd`` float32 [B, L]; with ``normalized`` also ``norm`` [B, L, 768], the
        normalized rows the next layer's residual add forms."""
        ids = np.ascontiguousarray(np.asarray(input_ids), dtype=np.int32)
        mask = np.ascontiguousarray(np.asarray(attention_mask), dtype=np.int32)
        B, L = ids.shape
        rows = np.empty((B, L, 768), np.float32)
        stats = np.empty((B, L, 2), np.float32)
        norm = np.empty((B, L, 768), np.float32) if normalized else None
        i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        _lib.check(_lib.lib().hac_encoder_layer_state(self._h, ids.ctypes.data_as(i32p), mask.ctypes.data_as(i32p), B, L, int(layer),
                                                      rows.ctypes.data_as(f32p), stats.ctypes.data_as(f32p),
                                                      norm.ctypes.data_as(f32p) if normalized else None))
        out = {"rows": rows, "mean": stats[..., 0], "rstd": stats[..., 1]}
        if normalized:
            out["norm"] = norm
        return out

    def eval(self):
        return self

    def to(self, device):
        return self

    def set_option(self, name, value):
        """Tuning / test switch of this handle (include/haconvdr.h: hac_encoder_set_option), e.g. ("gemm", "classic")."""
        _lib.check(_lib.lib().hac_encoder_set_option(self._h, str(name).encode(), str(value).encode()))
        if str(name) == "pooling":
            self._pooling = str(value)

    @property
    def use_mean(self):
        """The reference class's public switch (src/models.py:30, :52-61): False, the default, pools the <s> row
        (``emb_all[:, 0]``); True the masked mean of the last layer's rows over each sequence's attended tokens.  Setting it is
        ``set_option("pooling", "mean" | "first")``: the kernels run the last layer on every row in mean mode."""
        return self._pooling == "mean"

    @use_mean.setter
    def use_mean(self, value):
        self.set_option("pooling", "mean" if value else "first")

    def last_plan(self):
        """Kernel families of the most recent forward: "gemm=gemm8|classic256|classic128|split128 attn=... sub_batches=N rows=R ...",
        with " precision=split" appended when it ran in split mode, " pool=mean" when it pooled the masked mean and " model=bert"
        when the handle is a BERTEncoder."""
        return _lib.lib().hac_encoder_last_plan(self._h).decode()

    KERNEL_CLASSES = ("qkv", "attention", "out_proj", "ffn_up", "ffn_down", "layernorm")   # HAC_ENC_CLASS_* of include/haconvdr.h

    def set_profiling(self, on=True, classes=()):
        """hipEvent pairs around the layer stack of every forward (``on``) and around every launch of the named
        kernel classes (``classes``: names from KERNEL_CLASSES, or "all")."""
        if classes == "all":
            classes = self.KERNEL_CLASSES
        mask = int(bool(on))
        for c in classes:
            mask |= 2 << self.KERNEL_CLASSES.index(c)
        _lib.check(_lib.lib().hac_encoder_set_profiling(self._h, mask))

    def profile_drain(self, cap=4096):
        buf = (ctypes.c_float * cap)()
        n = ctypes.c_int()
        _lib.check(_lib.lib().hac_encoder_profile_drain(self._h, buf, cap, ctypes.byref(n)))
        return [float(buf[i]) for i in range(n.value)]

    def last_clock_mhz(self):
        """(shader clock in MHz, seconds) inside the most recent large-batch FFN-up launch made with class profiling on, or
        None (hac_encoder_last_clock): what fractions of a peak are normalised by across boxes that hold different clocks."""
        out = (ctypes.c_uint64 * 2)()
        _lib.check(_lib.lib().hac_encoder_last_clock(self._h, out))
        if not out[1]:
            return None
        return 100.0 * int(out[0]) / int(out[1]), int(out[1]) / 100e6

    def attention_redo(self):
        """How often the woven attention kernel handed an item to its fix-up pass in the most recent forward (upper bound of
        the items, 0 iff none; hac_encoder_attention_redo).  Test aid; waits for the device."""
        n = ctypes.c_longlong()
        _lib.check(_lib.lib().hac_encoder_attention_redo(self._h, ctypes.byref(n)))
        return int(n.value)

    def profile_drain_class(self, name, cap=16384):
        """Durations (ms, launch order) of the launches of one kernel class since the last drain."""
        buf = (ctypes.c_float * cap)()
        n = ctypes.c_int()
        _lib.check(_lib.lib().hac_encoder_profile_drain_class(self._h, self.KERNEL_CLASSES.index(name), buf, cap, ctypes.byref(n)))
        return [float(buf[i]) for i in range(n.value)]


class BERTEncoder(ANCEEncoder):
    """The reference's ``BERT`` class (src/models.py:66-110; load_model's BERT_Query / BERT_Passage): the same head, pooling and
    forward as ``ANCE`` over a ``BertModel``.  Checkpoint names are ``bert.*`` (``bert.pooler.*`` is unused by forward, like
    ``classifier.*``), position ids are ``arange(L)`` whatever the token ids, so the 512-row table serves L = 512, row 0 of the
    2-row token-type table is added (the reference never passes ``token_type_ids``) and the LayerNorm eps is BertConfig's
    1e-12.  Behind the embedding stage it runs the kernels ANCEEncoder runs (the handle's "model" option, include/haconvdr.h)."""
    MODEL = "bert"
    KEY_PREFIX = "bert."
    UNUSED_PREFIXES = ("classifier.", "bert.pooler.")
    CONFIG_DEFAULTS = {"ln_eps": 1e-12, "pad_token_id": 0}    # BertConfig's

    def __init__(self, n_layers=12, vocab=30522, max_pos=512, type_vocab=2, pad_token_id=0, ln_eps=1e-12, device=0, precision="bf16",
                 pooling="first"):
        super().__init__(n_layers=n_layers, vocab=vocab, max_pos=max_pos, type_vocab=type_vocab, pad_token_id=pad_token_id, ln_eps=ln_eps,
                         device=device, precision=precision, pooling=pooling)
