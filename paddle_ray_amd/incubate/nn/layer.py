"""Fused layer classes (parity: python/paddle/incubate/nn/layer/*)."""
import math

from ...nn.layer.layers import Layer
from ...nn import initializer as I
from . import functional as FF


class FusedLinear(Layer):
    def __init__(self, in_features, out_features, weight_attr=None, bias_attr=None,
                 transpose_weight=False, name=None):
        super().__init__()
        shape = [out_features, in_features] if transpose_weight else [in_features, out_features]
        self.weight = self.create_parameter(shape, weight_attr)
        self.bias = self.create_parameter([out_features], bias_attr, is_bias=True)
        self.transpose_weight = transpose_weight

    def forward(self, x):
        return FF.fused_linear(x, self.weight, self.bias, self.transpose_weight)


class FusedDropoutAdd(Layer):
    def __init__(self, p=0.5, mode="upscale_in_train", name=None):
        super().__init__()
        self.p, self.mode = p, mode

    def forward(self, x, y):
        return FF.fused_dropout_add(x, y, self.p, self.training, self.mode)


class FusedBiasDropoutResidualLayerNorm(Layer):
    def __init__(self, embed_dim, dropout_rate=0.5, weight_attr=None, bias_attr=None,
                 epsilon=1e-5, name=None):
        super().__init__()
        self.linear_bias = self.create_parameter([embed_dim], bias_attr, is_bias=True)
        self.ln_scale = self.create_parameter([embed_dim], weight_attr,
                                              default_initializer=I.Constant(1.0))
        self.ln_bias = self.create_parameter([embed_dim], bias_attr, is_bias=True)
        self.dropout_rate, self.epsilon = dropout_rate, epsilon

    def forward(self, x, residual):
        return FF.fused_bias_dropout_residual_layer_norm(x, residual, self.linear_bias,
                                                         self.ln_scale, self.ln_bias,
                                                         self.dropout_rate, self.epsilon,
                                                         self.training)


class FusedMultiHeadAttention(Layer):
    def __init__(self, embed_dim, num_heads, dropout_rate=0.5, attn_dropout_rate=0.5, kdim=None,
                 vdim=None, normalize_before=False, need_weights=False, qkv_weight_attr=None,
                 qkv_bias_attr=None, linear_weight_attr=None, linear_bias_attr=None,
                 pre_ln_scale_attr=None, pre_ln_bias_attr=None, ln_scale_attr=None,
                 ln_bias_attr=None, epsilon=1e-5, nranks=1, ring_id=-1, transpose_qkv_wb=False,
                 name=None):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = embed_dim // num_heads
        self.normalize_before, self.epsilon = normalize_before, epsilon
        self.dropout_rate, self.attn_dropout_rate = dropout_rate, attn_dropout_rate
        self.transpose_qkv_wb = transpose_qkv_wb
        qshape = [embed_dim, 3 * embed_dim] if transpose_qkv_wb else \
            [3, num_heads, self.head_dim, embed_dim]
        self.qkv_weight = self.create_parameter(qshape, qkv_weight_attr)
        self.qkv_bias = self.create_parameter([3 * embed_dim] if transpose_qkv_wb else
                                              [3, num_heads, self.head_dim], qkv_bias_attr,
                                              is_bias=True)
        self.linear_weight = self.create_parameter([embed_dim, embed_dim], linear_weight_attr)
        self.linear_bias = self.create_parameter([embed_dim], linear_bias_attr, is_bias=True)
        one = I.Constant(1.0)
        self.pre_ln_scale = self.create_parameter([embed_dim], pre_ln_scale_attr,
                                                  default_initializer=one)
        self.pre_ln_bias = self.create_parameter([embed_dim], pre_ln_bias_attr, is_bias=True)
        self.ln_scale = self.create_parameter([embed_dim], ln_scale_attr, default_initializer=one)
        self.ln_bias = self.create_parameter([embed_dim], ln_bias_attr, is_bias=True)

    def forward(self, query, key=None, value=None, attn_mask=None, cache=None):
        return FF.fused_multi_head_attention(
            query, self.qkv_weight, self.linear_weight, self.normalize_before, self.pre_ln_scale,
            self.pre_ln_bias, self.ln_scale, self.ln_bias, self.epsilon, self.qkv_bias,
            self.linear_bias, cache, attn_mask, self.dropout_rate, self.attn_dropout_rate,
            self.epsilon, self.training, num_heads=self.num_heads,
            transpose_qkv_wb=self.transpose_qkv_wb)


class FusedFeedForward(Layer):
    def __init__(self, d_model, dim_feedforward, dropout_rate=0.1, epsilon=1e-05,
                 activation="relu", act_dropout_rate=None, normalize_before=False,
                 linear1_weight_attr=None, linear1_bias_attr=None, linear2_weight_attr=None,
                 linear2_bias_attr=None, ln1_scale_attr=None, ln1_bias_attr=None,
                 ln2_scale_attr=None, ln2_bias_attr=None, nranks=1, ring_id=-1, name=None):
        super().__init__()
        self.dropout_rate = dropout_rate
        self.act_dropout_rate = dropout_rate if act_dropout_rate is None else act_dropout_rate
        self.activation, self.normalize_before, self.epsilon = activation, normalize_before, \
            epsilon
        self.linear1_weight = self.create_parameter([d_model, dim_feedforward], linear1_weight_attr)
        self.linear1_bias = self.create_parameter([dim_feedforward], linear1_bias_attr,
                                                  is_bias=True)
        self.linear2_weight = self.create_parameter([dim_feedforward, d_model], linear2_weight_attr)
        self.linear2_bias = self.create_parameter([d_model], linear2_bias_attr, is_bias=True)
        one = I.Constant(1.0)
        self.ln1_scale = self.create_parameter([d_model], ln1_scale_attr, default_initializer=one)
        self.ln1_bias = self.create_parameter([d_model], ln1_bias_attr, is_bias=True)
        self.ln2_scale = self.create_parameter([d_model], ln2_scale_attr, default_initializer=one)
        self.ln2_bias = self.create_parameter([d_model], ln2_bias_attr, is_bias=True)

    def forward(self, src, cache=None):
        return FF.fused_feedforward(src, self.linear1_weight, self.linear2_weight,
                                    self.linear1_bias, self.linear2_bias, self.ln1_scale,
                                    self.ln1_bias, self.ln2_scale, self.ln2_bias,
                                    self.act_dropout_rate, self.dropout_rate, self.activation,
                                    self.epsilon, self.epsilon, self.normalize_before,
                                    self.training)


class FusedTransformerEncoderLayer(Layer):
    def __init__(self, d_model, nhead, dim_feedforward, dropout_rate=0.1, activation="relu",
                 attn_dropout_rate=None, act_dropout_rate=None, normalize_before=False,
                 weight_attr=None, bias_attr=None):
        super().__init__()
        adr = dropout_rate if attn_dropout_rate is None else attn_dropout_rate
        self.fused_attn = FusedMultiHeadAttention(d_model, nhead, dropout_rate, adr,
                                                  normalize_before=normalize_before)
        self.ffn = FusedFeedForward(d_model, dim_feedforward, dropout_rate, activation=activation,
                                    act_dropout_rate=act_dropout_rate,
                                    normalize_before=normalize_before)

    def forward(self, src, src_mask=None, cache=None):
        return self.ffn(self.fused_attn(src, attn_mask=src_mask))


class FusedMultiTransformer(Layer):
    """Stack of pre/post-LN transformer layers for inference and generation, parameters in
    the reference layout (parity: python/paddle/incubate/nn/layer/fused_transformer.py
    FusedMultiTransformer): qkv [3, H, D, E], linear [E, E], ffn1 [E, F], ffn2 [F, E].
    ``forward(src, attn_mask, caches, ..., time_step)`` runs the context phase (caches
    filled in place) or, with ``time_step``, one decode step on the HIP cache kernel; there
    ``seq_lens`` ([B], cache positions already filled per sequence) makes the batch ragged.
    ``gqa_group_size`` = KVH > 0 is grouped-query attention with KVH K/V heads
    (``self.kv_num_heads``), each shared by ``num_heads / KVH`` query heads: qkv is
    [H + 2*KVH, D, E] (query heads, k heads, v heads), its bias [H + 2*KVH, D], and the caches
    are [2, B, KVH, max_len, D].
    ``uint8`` caches are the 8-bit KV cache: ``forward`` then takes the per-layer lists
    ``cache_k_quant_scales`` / ``cache_v_quant_scales`` (fp32 [KVH], or [B, KVH] per sequence;
    optional ``cache_*_dequant_scales``) and ``quant_round_type`` / ``quant_max_bound`` /
    ``quant_min_bound``, as ``fused_multi_transformer`` does.
    ``block_tables`` ([B, MB] integers, ``-1`` for no block) makes ``caches`` block pools
    [2, NB, KVH, BS, D] shared by the sequences: the context phase writes the prompt through the
    table and a decode step reads and appends through it (``fused_multi_transformer``)."""

    def __init__(self, embed_dim, num_heads, dim_feedforward, dropout_rate=0.0, activation="gelu",
                 normalize_before=True, ln_scale_attrs=None, ln_bias_attrs=None,
                 qkv_weight_attrs=None, qkv_bias_attrs=None, linear_weight_attrs=None,
                 linear_bias_attrs=None, ffn_ln_scale_attrs=None, ffn_ln_bias_attrs=None,
                 ffn1_weight_attrs=None, ffn1_bias_attrs=None, ffn2_weight_attrs=None,
                 ffn2_bias_attrs=None, epsilon=1e-5, num_layers=-1, nranks=1,
                 trans_qkvw=True, ring_id=-1, name=None, gqa_group_size=-1):
        super().__init__()
        if num_layers < 0:
            num_layers = len(qkv_weight_attrs) if isinstance(qkv_weight_attrs, (list, tuple)) else 1
        assert embed_dim % num_heads == 0
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = embed_dim // num_heads
        # grouped-query attention: gqa_group_size K/V heads, each shared by num_heads / it query heads
        self._gqa_group_size = int(gqa_group_size) if gqa_group_size and int(gqa_group_size) > 0 else -1
        self.kv_num_heads = self._gqa_group_size if self._gqa_group_size > 0 else num_heads
        if num_heads % self.kv_num_heads != 0:
            raise ValueError(f"FusedMultiTransformer: num_heads={num_heads} is not a multiple of "
                             f"gqa_group_size={gqa_group_size}")
        self.normalize_before, self._epsilon = normalize_before, epsilon
        self.dropout_rate, self.activation, self._trans_qkvw = dropout_rate, activation, trans_qkvw
        one = I.Constant(1.0)

        def attr(a, i):
            return a[i] if isinstance(a, (list, tuple)) else a
        names = ('ln_scales', 'ln_biases', 'qkv_weights', 'qkv_biases', 'linear_weights',
                 'linear_biases', 'ffn_ln_scales', 'ffn_ln_biases', 'ffn1_weights', 'ffn1_biases',
                 'ffn2_weights', 'ffn2_biases')
        for n in names:
            setattr(self, n, [])
        E, H, D, F = embed_dim, num_heads, self.head_dim, dim_feedforward
        qkv_shape = [3, H, D, E] if trans_qkvw else [E, 3, H, D]
        qkv_bias_shape = [3, H, D]
        if self._gqa_group_size > 0:     # head rows: H query heads, then the k heads, then the v heads
            N = H + 2 * self.kv_num_heads
            qkv_shape = [N, D, E] if trans_qkvw else [E, N, D]
            qkv_bias_shape = [N, D]
        for i in range(num_layers):
            specs = (
                ('ln_scales', [E], ln_scale_attrs, False, one),
                ('ln_biases', [E], ln_bias_attrs, True, None),
                ('qkv_weights', qkv_shape, qkv_weight_attrs, False, None),
                ('qkv_biases', qkv_bias_shape, qkv_bias_attrs, True, None),
                ('linear_weights', [E, E], linear_weight_attrs, False, None),
                ('linear_biases', [E], linear_bias_attrs, True, None),
                ('ffn_ln_scales', [E], ffn_ln_scale_attrs, False, one),
                ('ffn_ln_biases', [E], ffn_ln_bias_attrs, True, None),
                ('ffn1_weights', [E, F], ffn1_weight_attrs, False, None),
                ('ffn1_biases', [F], ffn1_bias_attrs, True, None),
                ('ffn2_weights', [F, E], ffn2_weight_attrs, False, None),
                ('ffn2_biases', [E], ffn2_bias_attrs, True, None))
            for n, shp, a, is_bias, init in specs:
                p = self.create_parameter(shp, attr(a, i), is_bias=is_bias, default_initializer=init)
                self.add_parameter(f'{n}_{i}', p)
                getattr(self, n).append(p)

    def forward(self, src, attn_mask=None, caches=None, pre_caches=None, rotary_embs=None,
                rotary_emb_dims=0, seq_lens=None, time_step=None, cache_k_quant_scales=None,
                cache_v_quant_scales=None, cache_k_dequant_scales=None, cache_v_dequant_scales=None,
                quant_round_type=1, quant_max_bound=127.0, quant_min_bound=-127.0,
                block_tables=None):
        return FF.fused_multi_transformer(
            src, self.ln_scales, self.ln_biases, self.qkv_weights, self.qkv_biases,
            self.linear_weights, self.linear_biases, self.ffn_ln_scales, self.ffn_ln_biases,
            self.ffn1_weights, self.ffn1_biases, self.ffn2_weights, self.ffn2_biases,
            pre_layer_norm=self.normalize_before, epsilon=self._epsilon, cache_kvs=caches,
            pre_caches=pre_caches, seq_lens=seq_lens, rotary_embs=rotary_embs,
            time_step=time_step, attn_mask=attn_mask, dropout_rate=self.dropout_rate,
            rotary_emb_dims=rotary_emb_dims, activation=self.activation, training=self.training,
            trans_qkvw=self._trans_qkvw, gqa_group_size=self._gqa_group_size,
            cache_k_quant_scales=cache_k_quant_scales, cache_v_quant_scales=cache_v_quant_scales,
            cache_k_dequant_scales=cache_k_dequant_scales,
            cache_v_dequant_scales=cache_v_dequant_scales, quant_round_type=quant_round_type,
            quant_max_bound=quant_max_bound, quant_min_bound=quant_min_bound,
            block_tables=block_tables)


class FusedMultiTransformerDecoder:
    """Serving loop for a ``FusedMultiTransformer``: persistent KV caches, a prefill call, and
    per-token decode steps replayed from ONE captured HIP graph (the decode-attention kernel
    reads the position from a device int32 counter that the graph itself advances), so a
    step costs one graph launch instead of ~10 kernel launches per layer.

        dec = FusedMultiTransformerDecoder(model, batch_size=8, max_seq_len=2048)
        h = dec.prefill(prompt_hidden)          # [B, S0, E], fills the caches
        for _ in range(n): h_t = dec.step(x_t)  # [B, 1, E] -> [B, 1, E]
    ``attn_mask`` (additive, [B, max_seq_len]) masks padded positions across all steps.

    Ragged batches: ``prefill(x, seq_lens=lens)`` takes right-padded prompts; every sequence
    then continues at its own position (``self.lens``, a device int32 [B] counter that the
    captured graph advances together with ``self.t`` = max(lens); only a ragged prefill
    makes it live), so one graph still serves the whole batch and a short sequence streams
    only its own part of the cache.
    ``set_rotary(cos, sin, rotary_emb_dims)`` installs [max_seq_len, D] rotary tables: prefill
    uses rows [0, S0), each step gathers every sequence's row by its current position.

    8-bit KV cache: ``kv_cache_dtype='int8'`` allocates ``uint8`` caches (half the bytes a
    bf16 cache streams per step and occupies per context; ``ops.fused.kv_quantize`` is the
    stored byte). ``cache_scales`` is a per-layer list of ``(k_quant, v_quant)`` fp32 [KVH]
    tensors, the static scales. With ``cache_scales=None`` the scales are dynamic: ``prefill``
    sets, per layer, sequence and K/V head, ``127 / absmax`` over the sequence's own valid
    prompt positions of K (after rotary) and of V (1 for an all-zero head); tokens decoded
    later saturate at the bounds. Either way the scales live in persistent device buffers
    (``self.kv_scales``, per layer fp32 [4, Bs, KVH] = k quant, v quant, k dequant, v dequant)
    that ``prefill`` fills before the graph is captured, so the one graph keeps serving every
    step. A dynamic ``prefill`` holds the prompt's K/V in the model dtype until it has the scales.

    Paged KV cache: ``block_size=BS`` replaces the per-slot ``max_seq_len`` rows by one block
    pool per layer, ``self.caches[i]`` [2, num_blocks, KVH, BS, D] (float or ``uint8``), shared by
    all slots through one persistent device table ``self.tables`` [B, MB] int32
    (``MB = ceil(max_seq_len / BS)``, ``-1`` = no block; ``num_blocks`` defaults to ``B * MB``,
    a smaller pool serves batches that never need every row at once). Blocks come from a host
    free list: ``prefill`` gives sequence ``b`` ``ceil(len_b / BS)`` blocks, and ``step`` gives a
    slot a new block when its position (a host mirror of ``self.lens``; the only sync is one in
    ``prefill`` for device ``seq_lens``) reaches a block boundary, by a small write into the
    table outside the graph, so the captured graph is never re-captured. ``free_blocks`` is the
    number of free blocks; a ``step`` or ``prefill`` that needs more raises ``RuntimeError``
    before it changes anything. Paged mode always runs the per-sequence (ragged) graph.
    Continuous batching: ``release(b)`` returns slot ``b``'s blocks, clears its table row and
    parks its position at ``MB * BS``, where the kernel's guard gives zeros and writes nothing;
    ``admit(b, x)`` (x [1, S, E]) allocates blocks, runs the context phase for that one prompt
    through table row ``b`` and sets the slot's position to ``S`` (and, with dynamic int8
    scales, the slot's scales from its prompt), leaving the other slots and the graph alone.
    On the GPU ``BS`` must be a power of two >= 16.

    Several tokens per step: ``step_multi(x)`` (x [B, T, E]) scores T new tokens per slot at the
    slots' current positions in one pass over the caches, equal to T ``step`` calls, writes
    their K/V and advances nothing; ``commit(accepted)`` then advances every slot by its own
    count in [0, T]. Rows written past the new position are dead: the next step overwrites them
    (paged: blocks already allocated stay with the slot). It always runs the per-sequence graph
    (a runner in uniform mode switches to it), one captured graph per T, and mixes freely with
    ``step``. Speculative decoding with a draft model proposing T - 1 tokens after the last
    accepted one:

        x = embed(last)                              # [B, 1, E]
        while not done:
            draft = propose(last, T - 1)             # [B, T - 1] token ids from the draft model
            toks = cat([last, draft], 1)             # [B, T]
            h = dec.step_multi(embed(toks))          # [B, T, E]: row j scores the token after toks[:, j]
            pred = head(h).argmax(-1)                # [B, T]; or pred = sampler(head(h)), see below
            ok = (pred[:, :-1] == draft).int().cumprod(1).sum(1)   # drafts accepted per slot
            dec.commit(ok + 1)                       # toks[:, :ok + 1] are now part of the sequence
            last = pred.gather(1, ok[:, None])       # the model's own next token
    With ``sampler = TokenSampler(B, temperature=..., top_k=..., top_p=...)`` (this package) in
    place of ``argmax``, row j's token is drawn with slot b's temperature / top-k / top-p in one
    kernel and no host sync (``top_k=1`` is the ``argmax`` above); a draft is then accepted when it
    equals the token drawn for its row.
    On the GPU T times the query heads per K/V head (T rounded up to a power of two) must not
    exceed 8 (``ops.fused.MULTI_MAX_ROWS``).
    """

    def __init__(self, model, batch_size, max_seq_len, use_graph=True, kv_cache_dtype=None,
                 cache_scales=None, block_size=None, num_blocks=None):
        import torch
        self.model = model
        self.B, self.L = int(batch_size), int(max_seq_len)
        p0 = model.qkv_weights[0]._t
        self.dev, self.dtype = p0.device, p0.dtype
        D, E = model.head_dim, model.embed_dim
        KVH = getattr(model, 'kv_num_heads', model.num_heads)    # grouped-query models cache KVH heads
        n = len(model.qkv_weights)
        if kv_cache_dtype not in (None, 'int8'):
            raise ValueError(f"FusedMultiTransformerDecoder: kv_cache_dtype must be None (the model "
                             f"dtype) or 'int8', got {kv_cache_dtype!r}")
        self.q8 = kv_cache_dtype == 'int8'
        if cache_scales is not None and not self.q8:
            raise ValueError("FusedMultiTransformerDecoder: cache_scales go with kv_cache_dtype='int8'")
        self.dynamic_scales = self.q8 and cache_scales is None
        self.kv_scales, self._qkw = None, {}
        if self.q8:
            Bs = self.B if self.dynamic_scales else 1
            self.kv_scales = [torch.ones(4, Bs, KVH, device=self.dev, dtype=torch.float32)
                              for _ in range(n)]
            if cache_scales is not None:
                if len(cache_scales) != n:
                    raise ValueError(f"FusedMultiTransformerDecoder: cache_scales has "
                                     f"{len(cache_scales)} entries for {n} layers")
                for s, pair in zip(self.kv_scales, cache_scales):
                    for j, q in enumerate(pair):
                        q = torch.as_tensor(q._t if hasattr(q, '_t') else q, dtype=torch.float32)
                        if tuple(q.shape) != (KVH,) or not bool((torch.isfinite(q) & (q > 0)).all()):
                            raise ValueError(f"FusedMultiTransformerDecoder: cache_scales holds per "
                                             f"layer (k_quant, v_quant), finite positive [{KVH}] "
                                             f"tensors; got {tuple(q.shape)}")
                        s[j, 0].copy_(q)
                        s[2 + j, 0].copy_(1.0 / q.to(self.dev))
            # views of the packed buffers: the decode wrapper finds them packed and copies nothing
            pick = (lambda s, j: s[j]) if self.dynamic_scales else (lambda s, j: s[j, 0])
            self._qkw = {name: [pick(s, j) for s in self.kv_scales] for j, name in enumerate(
                ('cache_k_quant_scales', 'cache_v_quant_scales', 'cache_k_dequant_scales',
                 'cache_v_dequant_scales'))}
        self.paged = block_size is not None
        if num_blocks is not None and not self.paged:
            raise ValueError("FusedMultiTransformerDecoder: num_blocks goes with block_size")
        shape = (2, self.B, KVH, self.L, D)
        if self.paged:
            self.BS = int(block_size)
            if self.BS < 1:
                raise ValueError(f"FusedMultiTransformerDecoder: block_size must be >= 1, got {block_size}")
            self.MB = -(-self.L // self.BS)
            self.NB = self.B * self.MB if num_blocks is None else int(num_blocks)
            if self.NB < 1:
                raise ValueError(f"FusedMultiTransformerDecoder: num_blocks must be >= 1, got {num_blocks}")
            shape = (2, self.NB, KVH, self.BS, D)
            self.tables = torch.full((self.B, self.MB), -1, dtype=torch.int32, device=self.dev)
            self._free = list(range(self.NB - 1, -1, -1))       # popped from the end: block 0 first
            self._blocks = [[] for _ in range(self.B)]           # host: each slot's blocks, in order
            self._pos = [0] * self.B                             # host mirror of self.lens; None: released
        # a uint8 cache starts at the byte of level 0
        self.caches = [torch.full(shape, 128, device=self.dev, dtype=torch.uint8) if self.q8 else
                       torch.zeros(shape, device=self.dev, dtype=self.dtype) for _ in range(n)]
        self.t = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.lens = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.ragged = self.paged      # paged mode: always the per-sequence graph
        self.rot = None               # [2, max_seq_len, D] fp32 (cos, sin)
        self.rot_dims = 0
        self.mask = torch.zeros(self.B, 1, 1, self.L, dtype=torch.float32, device=self.dev)
        self.x_buf = torch.zeros(self.B, 1, E, device=self.dev, dtype=self.dtype)
        self.use_graph = use_graph and self.dev.type == 'cuda'
        self._graph = None
        self._out = None
        self._multi = {}              # T -> [x buffer [B, T, E], captured graph, its output]
        self._last_T = None           # T of the step_multi that commit() may follow

    def _caches(self):
        from ...framework.core import Tensor
        return [Tensor(c) for c in self.caches]

    def set_mask(self, attn_mask):
        import torch
        m = attn_mask._t if hasattr(attn_mask, '_t') else torch.as_tensor(attn_mask)
        self.mask.copy_(m.reshape(self.B, 1, 1, self.L).to(self.mask.dtype))

    def set_rotary(self, cos, sin, rotary_emb_dims):
        """Rotary tables ``cos`` / ``sin`` [max_seq_len, D] (row p = position p) for prefill and
        every later step. Call it before ``prefill``: the step graph is captured with it."""
        import torch
        D = self.model.head_dim
        tab = torch.stack([torch.as_tensor(c._t if hasattr(c, '_t') else c).reshape(self.L, D)
                           for c in (cos, sin)])
        self.rot = tab.to(device=self.dev, dtype=torch.float32).contiguous()
        self.rot_dims = int(rotary_emb_dims)
        self._graph = None
        self._multi = {}

    def prefill(self, x, attn_mask=None, seq_lens=None):
        """Context phase over the prompt (caches filled in place); decode continues at S0, or
        with ``seq_lens`` ([B], right-padded prompts) at every sequence's own length."""
        from ...framework.core import Tensor
        import torch
        xt = x._t if hasattr(x, '_t') else x
        S0 = xt.shape[1]
        if attn_mask is None:
            m = torch.triu(torch.full((S0, S0), float('-inf'), device=self.dev), 1)
            attn_mask = Tensor(m.expand(self.B, 1, S0, S0).to(self.dtype))
        kw = {}
        if self.rot is not None:
            r = self.rot[:, :S0]                           # [2, S0, D], the same for every b
            kw = dict(rotary_embs=Tensor(r[:, None, None].expand(2, self.B, 1, S0, r.shape[-1])),
                      rotary_emb_dims=self.rot_dims)
        ragged = seq_lens is not None
        if ragged:
            sl = seq_lens._t if hasattr(seq_lens, '_t') else torch.as_tensor(seq_lens)
            sl = sl.reshape(self.B).to(device=self.dev, dtype=torch.int32)
            kw['seq_lens'] = Tensor(sl)
        if self.paged:
            self._assign([int(n) for n in sl.tolist()] if ragged else [S0] * self.B)
            kw['block_tables'] = Tensor(self.tables)
        with torch.no_grad():
            if self.dynamic_scales:
                # the prompt's K/V in the model dtype first: their absmax gives the scales
                KVH, D = self.caches[0].shape[2], self.caches[0].shape[4]
                tmp = [torch.zeros(2, self.B, KVH, S0, D, device=self.dev, dtype=self.dtype)
                       for _ in self.caches]
                out, _ = self.model(Tensor(xt), attn_mask=attn_mask, caches=[Tensor(c) for c in tmp],
                                    **{k: v for k, v in kw.items() if k != 'block_tables'})
                self._quantize_prompt(tmp, sl if ragged else None)
            else:
                out, _ = self.model(Tensor(xt), attn_mask=attn_mask, caches=self._caches(), **kw,
                                    **self._qkw)
        if ragged:
            self.lens.copy_(sl)
            self.t.copy_(sl.max().reshape(1))
        else:
            self.lens.fill_(S0)
            self.t.fill_(S0)
        if not self.paged and ragged != self.ragged:
            self.ragged, self._graph = ragged, None      # the other graph
        return out

    # ------------------------------------------------------------------ paged mode
    @property
    def free_blocks(self):
        """Number of blocks on the free list (paged mode)."""
        return len(self._free)

    def _need_paged(self, what):
        if not self.paged:
            raise RuntimeError(f"FusedMultiTransformerDecoder.{what} needs paged mode (block_size=...)")

    def _set_row(self, b, blocks):
        """Slot ``b``'s blocks on the host and its table row on the device (the rest -1)."""
        import torch
        self._blocks[b] = list(blocks)
        row = torch.full((self.MB,), -1, dtype=torch.int32)
        row[:len(blocks)] = torch.tensor(blocks, dtype=torch.int32)
        self.tables[b].copy_(row)

    def _assign(self, lens):
        """A fresh batch: every block back on the free list, then ``ceil(len_b / BS)`` blocks for
        each sequence. Raises before it changes anything when the pool is too small."""
        need = [-(-n // self.BS) for n in lens]
        if any(not 0 <= n <= self.MB * self.BS for n in lens):
            raise ValueError(f"FusedMultiTransformerDecoder: prompt lengths {lens} outside "
                             f"[0, {self.MB * self.BS}]")
        if sum(need) > self.NB:
            raise RuntimeError(f"FusedMultiTransformerDecoder: the prompts need {sum(need)} blocks of "
                               f"{self.BS}, the pool has {self.NB}")
        self._free = list(range(self.NB - 1, -1, -1))
        for b, k in enumerate(need):
            self._set_row(b, [self._free.pop() for _ in range(k)])
        self._pos = list(lens)

    def _grow(self):
        """Before a step: a live slot whose position starts a block it does not have yet gets one,
        written into the device table outside the graph. Raises before it changes anything."""
        want = [b for b, p in enumerate(self._pos)
                if p is not None and p < self.L and p // self.BS >= len(self._blocks[b])]
        if len(want) > len(self._free):
            raise RuntimeError(f"FusedMultiTransformerDecoder: {len(want)} slots need a new block and "
                               f"{len(self._free)} are free; release a slot or use a larger pool")
        for b in want:
            e = self._free.pop()
            self.tables[b, len(self._blocks[b])].fill_(e)
            self._blocks[b].append(e)

    def _grow_multi(self, T):
        """Before a multi-token step: every live slot gets the blocks that cover [p, p + T).
        Raises before it changes anything when the free list is too short."""
        cap = self.MB * self.BS
        want = [(b, (min(p + T, cap) - 1) // self.BS + 1 - len(self._blocks[b]))
                for b, p in enumerate(self._pos) if p is not None and p < self.L]
        want = [(b, k) for b, k in want if k > 0]
        if sum(k for _, k in want) > len(self._free):
            raise RuntimeError(f"FusedMultiTransformerDecoder: {T} tokens per slot need "
                               f"{sum(k for _, k in want)} new blocks and {len(self._free)} are free; "
                               "release a slot or use a larger pool")
        for b, k in want:
            for _ in range(k):
                e = self._free.pop()
                self.tables[b, len(self._blocks[b])].fill_(e)
                self._blocks[b].append(e)

    def release(self, b):
        """Slot ``b`` leaves the batch: its blocks go back to the free list, its table row to -1
        and its position to ``MB * BS``, where every later step gives it zeros and writes nothing."""
        self._need_paged('release')
        b = int(b)
        self._free.extend(reversed(self._blocks[b]))
        self._set_row(b, [])
        self.lens[b].fill_(self.MB * self.BS)
        self._pos[b] = None

    def admit(self, b, x, attn_mask=None):
        """A new prompt ``x`` [1, S, E] joins the running batch in the released (or unused) slot
        ``b``: blocks are allocated, the context phase runs for this one sequence through table
        row ``b`` and the slot continues at position ``S``. Returns the prompt's output
        [1, S, E]; the other slots and the captured step graph are untouched."""
        from ...framework.core import Tensor
        import torch
        self._need_paged('admit')
        b = int(b)
        xt = x._t if hasattr(x, '_t') else x
        S = xt.shape[1]
        if xt.shape[0] != 1 or not 0 < S <= self.L:
            raise ValueError(f"FusedMultiTransformerDecoder.admit: x must be [1, S, E] with "
                             f"0 < S <= {self.L}, got {tuple(xt.shape)}")
        if self._blocks[b]:
            raise RuntimeError(f"FusedMultiTransformerDecoder.admit: slot {b} holds a sequence; "
                               "release it first")
        need = -(-S // self.BS)
        if need > len(self._free):
            raise RuntimeError(f"FusedMultiTransformerDecoder.admit: the prompt needs {need} blocks "
                               f"and {len(self._free)} are free")
        self._set_row(b, [self._free.pop() for _ in range(need)])
        if attn_mask is None:
            m = torch.triu(torch.full((S, S), float('-inf'), device=self.dev), 1)
            attn_mask = Tensor(m.expand(1, 1, S, S).to(self.dtype))
        kw = dict(block_tables=Tensor(self.tables[b:b + 1]))
        if self.rot is not None:
            r = self.rot[:, :S]
            kw.update(rotary_embs=Tensor(r[:, None, None]), rotary_emb_dims=self.rot_dims)
        with torch.no_grad():
            if self.dynamic_scales:
                KVH, D = self.caches[0].shape[2], self.caches[0].shape[4]
                tmp = [torch.zeros(2, 1, KVH, S, D, device=self.dev, dtype=self.dtype) for _ in self.caches]
                out = self.model(Tensor(xt), attn_mask=attn_mask, caches=[Tensor(c) for c in tmp],
                                 **{k: v for k, v in kw.items() if k != 'block_tables'})[0]
                self._quantize_prompt(tmp, None, slot=b)
            else:
                out, _ = self.model(Tensor(xt), attn_mask=attn_mask, caches=self._caches(), **kw,
                                    **self._qkw)
        self.lens[b].fill_(S)
        self.t.copy_(torch.clamp(self.t, min=S))
        self._pos[b] = S
        return out

    def _quantize_prompt(self, kv, seq_lens, slot=None):
        """Dynamic scales from the prompt's K/V (``kv``: per layer [2, B, KVH, S0, D], K after
        rotary) over each sequence's valid positions, written into ``self.kv_scales``; then
        the quantised prompt into the uint8 caches (paged: through the table). ``slot``: ``kv``
        holds that one slot's prompt (batch 1) and only its scales and blocks are written."""
        import torch
        from ...ops import fused as K
        rows = slice(None) if slot is None else slice(slot, slot + 1)
        S0 = kv[0].shape[3]
        pad = None
        if seq_lens is not None:
            pad = (torch.arange(S0, device=self.dev)[None, :] >= seq_lens[:, None].to(self.dev))
            pad = pad[None, :, None, :, None]
        for s, c, x in zip(self.kv_scales, self.caches, kv):
            a = x.float().abs()
            if pad is not None:
                a = a.masked_fill(pad, 0.0)
            a = a.amax(dim=(3, 4))                            # [2, B, KVH]
            q = torch.where(a > 0, 127.0 / a, torch.ones_like(a))
            s[:2, rows].copy_(q)
            s[2:, rows].copy_(1.0 / q)
            if self.paged:
                FF._scatter_paged(c, self.tables[rows], K.kv_quantize(x[0], s[0, rows]),
                                  K.kv_quantize(x[1], s[1, rows]))
            else:
                c[0, :, :, :S0] = K.kv_quantize(x[0], s[0])
                c[1, :, :, :S0] = K.kv_quantize(x[1], s[1])

    def _step_eager(self):
        from ...framework.core import Tensor
        kw = dict(self._qkw)
        if self.ragged:
            kw['seq_lens'] = Tensor(self.lens)
        if self.paged:
            kw['block_tables'] = Tensor(self.tables)
        if self.rot is not None:
            # every sequence's own row: its position when ragged, else the common one
            pos = self.lens if self.ragged else self.t
            if self.paged:            # a released slot is parked past the tables: any row will do
                pos = pos.clamp(max=self.L - 1)
            r = self.rot.index_select(1, pos)
            r = r.expand(2, self.B, r.shape[-1])
            kw.update(rotary_embs=Tensor(r[:, :, None, None]), rotary_emb_dims=self.rot_dims)
        out, _ = self.model(Tensor(self.x_buf), attn_mask=Tensor(self.mask), caches=self._caches(),
                            time_step=Tensor(self.t), **kw)
        return out._t

    def _step_multi_eager(self, T):
        import torch
        from ...framework.core import Tensor
        kw = dict(self._qkw)
        kw['seq_lens'] = Tensor(self.lens)
        if self.paged:
            kw['block_tables'] = Tensor(self.tables)
        if self.rot is not None:
            # token j of a slot: the row of its position + j (a parked or full slot is guarded:
            # any row will do)
            pos = (self.lens[:, None] + torch.arange(T, device=self.dev, dtype=torch.int32)[None, :]
                   ).clamp(max=self.L - 1)
            r = self.rot.index_select(1, pos.reshape(-1)).view(2, self.B, 1, T, -1)
            kw.update(rotary_embs=Tensor(r), rotary_emb_dims=self.rot_dims)
        out, _ = self.model(Tensor(self._multi[T][0]), attn_mask=Tensor(self.mask), caches=self._caches(),
                            time_step=Tensor(self.t), **kw)
        return out._t

    def step_multi(self, x):
        """T tokens for every sequence (x [B, T, E]) at the slots' current positions, in one pass
        over the caches: returns [B, T, E], row j what the j-th of T ``step`` calls would return.
        The K/V of all T tokens are written; no position advances until ``commit``."""
        import torch
        from ...framework.core import Tensor
        xt = x._t if hasattr(x, '_t') else x
        if xt.dim() != 3 or xt.shape[0] != self.B or xt.shape[1] < 1:
            raise ValueError(f"FusedMultiTransformerDecoder.step_multi: x must be [{self.B}, T, E] with "
                             f"T >= 1, got {tuple(xt.shape)}")
        T = int(xt.shape[1])
        if self.paged:                # blocks first: an exhausted pool raises with nothing changed
            self._grow_multi(T)
        if not self.ragged:           # every slot continues from the common position, on its own
            self.lens.copy_(self.t.expand(self.B))
            self.ragged, self._graph = True, None
        if T not in self._multi:
            self._multi[T] = [torch.zeros(self.B, T, xt.shape[2], device=self.dev, dtype=self.dtype),
                              None, None]
        ent = self._multi[T]
        ent[0].copy_(xt)
        self._last_T = T
        with torch.no_grad():
            if not self.use_graph:
                return Tensor(self._step_multi_eager(T))
            if ent[1] is None:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):  # warm-up (writes the same T cache rows, nothing advances)
                    self._step_multi_eager(T)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    ent[2] = self._step_multi_eager(T)
                ent[1] = g
            ent[1].replay()
        return Tensor(ent[2].clone())

    def commit(self, accepted):
        """After ``step_multi``: slot ``b`` keeps the first ``accepted[b]`` (in [0, T]) of its T
        tokens and continues behind them. ``accepted`` is a list, array or tensor of B counts (a
        tensor costs one sync, for the host mirror of the positions)."""
        import torch
        if self._last_T is None:
            raise RuntimeError("FusedMultiTransformerDecoder.commit follows a step_multi")
        a = accepted._t if hasattr(accepted, '_t') else accepted
        host = [int(n) for n in (a.reshape(-1).tolist() if isinstance(a, torch.Tensor)
                                 else torch.as_tensor(a).reshape(-1).tolist())]
        if len(host) != self.B or not all(0 <= n <= self._last_T for n in host):
            raise ValueError(f"FusedMultiTransformerDecoder.commit: need {self.B} counts in "
                             f"[0, {self._last_T}], got {host}")
        if self.paged:                # a released slot stays parked
            host = [0 if p is None else n for n, p in zip(host, self._pos)]
            self._pos = [p if p is None else p + n for n, p in zip(host, self._pos)]
            live = [p for p in self._pos if p is not None]
            self.lens.add_(torch.tensor(host, dtype=torch.int32).to(self.dev))
            self.t.fill_(max(live) if live else 0)
        else:
            self.lens.add_(torch.tensor(host, dtype=torch.int32).to(self.dev))
            self.t.copy_(self.lens.max().reshape(1))
        self._last_T = None

    def _advance(self):
        self.t.add_(1)
        if self.ragged:               # the uniform graph stays as it was: one counter
            self.lens.add_(1)

    def step(self, x_tok):
        """One token for every sequence: returns [B, 1, E]; the position advances by one."""
        import torch
        from ...framework.core import Tensor
        xt = x_tok._t if hasattr(x_tok, '_t') else x_tok
        if self.paged:                # blocks first: an exhausted pool raises with nothing changed
            self._grow()
            self._pos = [p if p is None else p + 1 for p in self._pos]
        self.x_buf.copy_(xt.reshape(self.x_buf.shape))
        with torch.no_grad():
            if not self.use_graph:
                out = self._step_eager()
                self._advance()
                return Tensor(out)
            if self._graph is None:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):  # warm-up (rewrites the same cache slot, t unchanged)
                    self._step_eager()
                torch.cuda.current_stream().wait_stream(s)
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph):
                    self._out = self._step_eager()
                    self._advance()
            self._graph.replay()
        return Tensor(self._out.clone())


class FusedEcMoe(Layer):
    def __init__(self, hidden_size, inter_size, num_experts, act_type, weight_attr=None,
                 bias_attr=None):
        super().__init__()
        self.bmm_weight0 = self.create_parameter([num_experts, hidden_size, inter_size],
                                                 weight_attr)
        self.bmm_bias0 = self.create_parameter([num_experts, 1, inter_size], bias_attr,
                                               is_bias=True)
        self.bmm_weight1 = self.create_parameter([num_experts, inter_size, hidden_size],
                                                 weight_attr)
        self.bmm_bias1 = self.create_parameter([num_experts, 1, hidden_size], bias_attr,
                                               is_bias=True)
        self.act_type = act_type

    def forward(self, x, gate):
        return FF.fused_ec_moe(x, gate, self.bmm_weight0, self.bmm_bias0, self.bmm_weight1,
                               self.bmm_bias1, self.act_type)
