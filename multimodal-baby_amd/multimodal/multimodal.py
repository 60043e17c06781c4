"""CVCL model classes with the reference's surface, computed by libcvcl_hip (MI355X).

Same class names, constructor signatures, ``add_to_argparse`` flags, return tuples and parameter names as
the reference ``multimodal/multimodal.py`` (VisionEncoder :56-194, TextEncoder :278-688, MultiModalModel
:691-822, LanguageModel :825-960) for the flat / contrastive path; every arithmetic step is a HIP kernel
reached through the C ABI (``ops.py`` / ``resnext.py`` / ``vision_transformer_dino_mugs.py``).  Branches
the contrastive configurations never take (spatial similarity, cbow, captioning/attention LM, beam
search) raise NotImplementedError instead of silently falling back to PyTorch ops.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops, parallel, resnext, text_train
from ._hip import CvclError
from .attention_maps import Hook
from .multimodal_data_module import EOS_TOKEN_ID, MAX_LEN_UTTERANCE, PAD_TOKEN_ID, SOS_TOKEN_ID
from .trunk_runtime import fingerprint, runtime_of, strip
from .utils import load_model

TEXT_ENCODER = "embedding"
ATTENTION_ACTIVATION = "relu"
EMBEDDING_TYPE = "flat"
EMBEDDING_DIM = 128
CRANGE = 1
DROPOUT_I = 0.0
DROPOUT_O = 0.0
PRETRAINED_CNN = True
FINETUNE_CNN = False
NORMALIZE_FEATURES = False
SIM = "max"
TEMPERATURE = 0.07
FIX_TEMPERATURE = False
CNN_MODEL = "models/TC-S-resnext.tar"
CNN_DINO = False
VIT_DINO = False
POS_EMBED_TYPE = "no_pos_embed"

_TORCHVISION_MODELS = {"resnext50_32x4d": resnext.resnext50_32x4d}

# Registration epoch: advanced whenever ANY nn.Module registers a parameter or a sub-module (torch's global registration hooks:
# ``m.x = Parameter / Module``, ``register_parameter``, ``add_module``, ``load_state_dict(assign=True)``).  VisionEncoder's eval
# graph cache keeps its parameter list only while the epoch stands still (see ``_graph_forward``).
_REGISTRATIONS = [0]


def _note_registration(*_a):
    _REGISTRATIONS[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_note_registration)
torch.nn.modules.module.register_module_module_registration_hook(_note_registration)


def set_parameter_requires_grad(model, feature_extracting=True):
    if feature_extracting:
        for param in model.parameters():
            param.requires_grad = False


class _EvalGraphs:
    """VisionEncoder's HIP-graph state: the switch (None = $CVCL_EVAL_GRAPH decides), the captured entries per input shape and the
    cached parameter list their fingerprints are taken over."""

    def __init__(self):
        self.on, self.entries, self.params = None, {}, None

    def drop(self, graphs=True):
        if graphs:
            self.entries = {}
        self.params = None


class VisionEncoder(nn.Module):
    """ResNeXt-50 / DINO ViT image encoder + linear projection to the embedding space."""

    def __init__(self, args):
        super().__init__()
        self.args = vars(args) if args is not None else {}
        self.embedding_type = self.args.get("embedding_type")
        self.embedding_dim = self.args.get("embedding_dim")
        self.pretrained_cnn = self.args.get("pretrained_cnn")
        self.cnn_model = self.args.get("cnn_model", CNN_MODEL)
        self.cnn_dino = self.args.get("cnn_dino", CNN_DINO)
        self.vit_dino = self.args.get("vit_dino", VIT_DINO)
        self.finetune_cnn = self.args.get("finetune_cnn")
        self._eval_graphs = _EvalGraphs()                     # never pickled
        self.model = self._load_pretrained_cnn()

    @staticmethod
    def add_to_argparse(parser):
        parser.add_argument("--pretrained_cnn", action="store_true", help="use pretrained CNN")
        parser.add_argument("--cnn_model", type=str, default=CNN_MODEL)
        parser.add_argument("--cnn_dino", action="store_true", default=CNN_DINO)
        parser.add_argument("--vit_dino", action="store_true", default=VIT_DINO)
        parser.add_argument("--finetune_cnn", action="store_true")

    def forward(self, x):
        if self._graph_eligible(x):
            return self._graph_forward(x)
        return self._eager_forward(x)

    def _eager_forward(self, x):
        if getattr(self, "vit_dino", False):
            cls = self.model(x)                               # pre-head cls token (reference :91)
            return ops.linear_f32(cls, self.model.head.weight, self.model.head.bias, split=self._head_split()), None   # reference :92
        layer = self.model[-2] if self.embedding_type == "spatial" else self.model.layer4     # reference :96-99
        with Hook(layer, requires_grad=False) as hook:                # reference :100-102
            features = self.model(x)
            feature_map = hook.activation
        return features, feature_map

    def _head_split(self) -> bool:
        """Arithmetic of the ViT head's fp32 GEMM, decided once per module so that EVERY call site of the layer (batched forward,
        one-image-at-a-time forward, graph replay) runs the same kernel and tests/test_batching-style comparisons stay bit-level:
        split-bf16 products in the bf16 compute mode, the exact fp32 MFMA otherwise (the parity mode)."""
        return getattr(self.model, "compute_dtype", None) == torch.bfloat16

    # ---- evaluation callers (eval.py:196-232, analysis loops calling encode_image one frame at a time): HIP-graph replay ----
    # An eval-mode, no-grad pass is ~66 (ResNeXt) / ~110 (ViT) small dependent launches; the host's launch lead is 0.15-0.2 ms of a
    # 0.8-1.4 ms call at B = 1..4 (profiles/r03_eval_latency.txt).  Opt-in (``enable_hip_graphs()`` or $CVCL_EVAL_GRAPH=1): the
    # pass is captured once per input shape into a HIP graph (torch.cuda.CUDAGraph = hipGraph on ROCm) over a static input buffer and
    # replayed; results are copies of the static outputs, bit-identical to the eager launches.  A graph replays the weight buffers
    # that were PACKED when it was captured, so every entry carries the fingerprint of the trunk's parameters it was captured
    # with ((data_ptr, _version) per parameter -- the key the eager path's own pack caches use) and is re-captured when that
    # changes: an in-place edit in eval mode, ``load_state_dict`` on this module or on any parent (``lit.load_state_dict`` recurses
    # through ``_load_from_state_dict`` and never calls the child's ``load_state_dict``), an optimizer step.  ``train()`` and the
    # two load paths also drop the graphs outright.
    def enable_hip_graphs(self, on: bool = True):
        self._eval_graphs.on, self._eval_graphs.entries = bool(on), {}
        return self

    @property
    def _graphs(self):
        """The captured entries, keyed by (input shape, device, compute dtype, trunk arithmetic)."""
        return self._eval_graphs.entries

    def _trunk_runtime(self):
        return runtime_of(getattr(self.model, "_resnet", self.model))     # (spatial embeddings: the Sequential wraps the ResNet that owns it)

    def _graph_eligible(self, x):
        on = self._eval_graphs.on
        if on is None:
            on = os.environ.get("CVCL_EVAL_GRAPH") == "1"
        return bool(on and not self.training and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
                    and self._trunk_runtime().stream is None and not torch.cuda.is_current_stream_capturing())

    def _graph_forward(self, x):
        state = self._eval_graphs
        graphs = state.entries
        key = (tuple(x.shape), str(x.device), getattr(self.model, "compute_dtype", None), getattr(self.model, "trunk_arithmetic", None))
        # (the parameter LIST is cached: the module-tree walk of ~160 parameters cost more host time per call than reading their
        # pointers and versions.  It is valid while no nn.Module anywhere registered a parameter or a sub-module since it was
        # taken -- ``model.fc = nn.Linear(...)``, ``load_state_dict(assign=True)``, ``register_parameter`` all pass torch's
        # global registration hooks, which advance _REGISTRATIONS; in-place edits and ``.data`` swaps show in the fingerprint)
        plist = state.params
        if plist is None or plist[0] != _REGISTRATIONS[0]:
            plist = state.params = (_REGISTRATIONS[0], list(self.model.parameters()))
        fp = fingerprint(plist[1])
        entry = graphs.get(key)
        if entry is not None and entry[5] != fp:              # weights changed since the capture: the packed copies are stale
            entry = None
            graphs.pop(key)
        if entry is None:
            cur = torch.cuda.current_stream(x.device)
            static_x = x.detach().clone().contiguous()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):                             # warm-up off the capture: weight packing, workspaces,
                for _ in range(2):                                    # kernel attributes
                    self._eager_forward(static_x)
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                feats, fmap = self._eager_forward(static_x)
            # (the trunk's cached workspaces are referenced by the graph: keep them alive whatever other shapes run later)
            entry = graphs[key] = (graph, static_x, feats, fmap, self._trunk_runtime().keep_alive(), fp)
        graph, static_x, feats, fmap, _keep, _fp = entry
        static_x.copy_(x, non_blocking=True)
        graph.replay()
        return feats.clone(), (fmap.clone() if fmap is not None else None)

    def train(self, mode: bool = True):
        self._eval_graphs.drop(graphs=mode)
        return super().train(mode)

    def load_state_dict(self, *a, **k):
        self._eval_graphs.drop()
        return super().load_state_dict(*a, **k)

    def _load_from_state_dict(self, *a, **k):                 # a parent's load_state_dict reaches this module here, not above
        self._eval_graphs.drop()
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):                            # .to() / .cuda() / .float(): new storage, maybe new Parameter objects
        self._eval_graphs.drop()
        return super()._apply(fn, *a, **k)

    def __getstate__(self):                                   # (checkpoints pickle whole encoders: graphs are never part of them)
        return strip(self.__dict__, "_eval_graphs")           # (__dict__: the instance's own state is what pickles)

    def __setstate__(self, d):                                # (also pickles of the reference's class and of earlier versions of this one)
        super().__setstate__(strip(d, "_eval_graphs"))
        self._eval_graphs = _EvalGraphs()

    def _forward_unbatched(self, x):
        """reference :106-114: one image at a time through self.model (what tests/test_batching.py compares with)."""
        outs = []
        for i in x:
            out = self.model(i.unsqueeze(0))
            if getattr(self, "vit_dino", False):
                out = ops.linear_f32(out, self.model.head.weight, self.model.head.bias, split=self._head_split())
            outs.append(out.squeeze(0))
        return torch.stack(outs)

    @property
    def last_cnn_out_dim(self):
        return 768 if self.vit_dino else 2048

    def set_compute_dtype(self, dtype, trunk_arithmetic="exact"):
        """Storage dtype of the encoder; trunk_arithmetic "split" (fp32 storage, ResNeXt only) forms the trunk's convolution
        products from split-bf16 parts -- the "32-split" precision.  The ViT and --finetune_cnn have no split form: refused here."""
        if trunk_arithmetic not in ("exact", "split"):
            raise ValueError(f"trunk_arithmetic must be 'exact' or 'split', got {trunk_arithmetic!r}")
        if trunk_arithmetic == "split":
            if dtype != torch.float32:
                raise CvclError("the 32-split precision stores fp32")
            if getattr(self, "vit_dino", False):
                raise CvclError("the 32-split precision exists for the ResNeXt encoders only, not the ViT (use 32 or bf16)")
            if getattr(self, "finetune_cnn", False):
                raise CvclError("--finetune_cnn is not available in the 32-split precision (use 32 or bf16)")
        self.model.compute_dtype = dtype
        if trunk_arithmetic == "split" or hasattr(self.model, "trunk_arithmetic"):
            self.model.trunk_arithmetic = trunk_arithmetic

    def _load_pretrained_cnn(self):
        if self.cnn_dino:
            print("Loading DINO resnext model!")
            model = load_model("dino_sfp_resnext50", self.pretrained_cnn)
        elif self.vit_dino:
            print("Loading DINO vision transformer model!")
            model = load_model("dino_sfp_vitb14", self.pretrained_cnn)
        else:
            name, checkpoint_path = self.cnn_model, None
            if name not in _TORCHVISION_MODELS:
                checkpoint_path = self.cnn_model
                if "resnext" not in name:
                    raise AssertionError(f"Unable to recognize the model name of {name}")
                name = "resnext50_32x4d"
            model = _TORCHVISION_MODELS[name](pretrained=bool(self.pretrained_cnn and not checkpoint_path))
            model.fc = nn.Linear(self.last_cnn_out_dim, 2765, bias=True)
            if self.pretrained_cnn and checkpoint_path:
                print("Loading pretrained CNN!")
                ckpt = torch.load(checkpoint_path, map_location="cpu")
                model.load_state_dict({k[len("module."):]: v for k, v in ckpt["model_state_dict"].items()})
        if not self.finetune_cnn:
            print("Freezing CNN layers!")
            set_parameter_requires_grad(model)
        else:
            print("Fine-tuning CNN layers!")
        if self.embedding_type == "spatial":                          # reference :181-185
            if self.vit_dino:
                raise NotImplementedError("spatial embeddings are defined for the CNN encoders only")
            from .resnext import SpatialResNet
            model = SpatialResNet(model, self.embedding_dim)
        elif self.embedding_type == "flat":
            print("Adding linear layer to vision encoder!")
            if self.vit_dino:
                model.head = nn.Linear(self.last_cnn_out_dim, self.embedding_dim)
            else:
                model.fc = nn.Linear(self.last_cnn_out_dim, self.embedding_dim)
        return model


class LockedDropout(nn.Module):
    """Dropout mask shared along ``dim`` (reference :46-53).  Identity in eval mode / p = 0."""

    def forward(self, x, dropout, dim=1):
        if not (self.training and dropout):
            return x
        if dim != 1 or x.dim() != 3:
            raise NotImplementedError("LockedDropout is used with [B, L, E] inputs and dim=1 on the contrastive path")
        B, L, E = x.shape
        y = text_train.DropoutAdd.apply(x.reshape(B * L, E), None, float(dropout), text_train._seed(), L, E)
        return y.view(B, L, E)


class TextEncoder(nn.Module):
    """Embedding mean-pool / LSTM / one-layer transformer text encoder."""

    def __init__(self, vocab, image_feature_map_dim, args):
        super().__init__()
        self.args = vars(args) if args is not None else {}
        self.text_encoder = self.args.get("text_encoder")
        self._captioning = self.args.get("captioning", False)
        self._attention = self.args.get("attention", False)
        self._attention_gate = self.args.get("attention_gate", False)
        self.embedding_type = self.args.get("embedding_type")
        self.embedding_dim = self.args.get("embedding_dim")
        self.hidden_dim = self.embedding_dim
        self.input_dim = self.embedding_dim
        self.crange = self.args.get("crange")
        self.dropout_i = self.args.get("dropout_i")
        self.dropout_o = self.args.get("dropout_o")
        self.pos_embed_type = self.args.get("pos_embed_type", POS_EMBED_TYPE)
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if self._attention:
            raise NotImplementedError("attention language models are outside the implemented path")
        self.vocab = vocab
        self.word2idx = self.vocab
        self.idx2word = {idx: word for word, idx in self.vocab.items()}
        self.embedding = nn.Embedding(self.vocab_size, self.embedding_dim, padding_idx=0)
        if self.text_encoder in ("lstm", "bilstm"):
            self.lstm = nn.LSTM(self.input_dim, self.hidden_dim, bidirectional=self.text_encoder == "bilstm")
        elif self.text_encoder == "transformer":
            print("Building transformer text encoder!")
            import copy
            self.encoder_layer = nn.TransformerEncoderLayer(d_model=self.embedding_dim, nhead=8)
            # reference :322 -- nn.TransformerEncoder deep-copies the layer, leaving `encoder_layer.*` as a
            # dead duplicate parameter set in the state_dict; kept for checkpoint parity
            self.transformer_encoder = nn.Module()
            self.transformer_encoder.layers = nn.ModuleList([copy.deepcopy(self.encoder_layer)])
            if self.pos_embed_type == "sinusoidal":
                pe = torch.zeros(MAX_LEN_UTTERANCE, self.embedding_dim)
                position = torch.arange(0, MAX_LEN_UTTERANCE).unsqueeze(1)
                div = torch.exp(torch.arange(0, self.embedding_dim, 2) * -(math.log(10000.0) / self.embedding_dim))
                pe[:, 0::2] = torch.sin(position * div)
                pe[:, 1::2] = torch.cos(position * div)
                self.register_buffer("pos_embed", pe.unsqueeze(1))
            elif self.pos_embed_type == "learned":
                self.pos_embed = nn.Parameter(torch.zeros(MAX_LEN_UTTERANCE, 1, self.embedding_dim))
        if self._captioning:                                                # reference :346-353
            assert self.regressional, "only regressional text encoder supports captioning"
            self.connector = nn.Linear(self.embedding_dim, 2 * self.lstm.num_layers * self.hidden_dim)
        self.lockdrop = LockedDropout()
        self.output_dropout = nn.Dropout(self.dropout_o)

    @staticmethod
    def add_to_argparse(parser):
        parser.add_argument("--text_encoder", type=str, default=TEXT_ENCODER,
                            choices=["embedding", "cbow", "lstm", "bilstm", "transformer"])
        parser.add_argument("--captioning", action="store_true")
        parser.add_argument("--attention", action="store_true")
        parser.add_argument("--attention_activation", type=str, default=ATTENTION_ACTIVATION, choices=["relu", "tanh"])
        parser.add_argument("--attention_gate", action="store_true")
        parser.add_argument("--crange", type=int, default=CRANGE)
        parser.add_argument("--dropout_i", type=float, default=DROPOUT_I)
        parser.add_argument("--dropout_o", type=float, default=DROPOUT_O)
        parser.add_argument("--pos_embed_type", type=str, default=POS_EMBED_TYPE,
                            choices=["no_pos_embed", "sinusoidal", "learned"])

    def initial_state(self, image_features):
        """Captioning: the LSTM's (h0, c0), each [B, H], from flat image features [B, E] through the connector (reference
        init_hidden :671-688: connector(f).reshape(B, 2, 1, H).permute(1, 2, 0, 3) -> h0 = out[:, :H], c0 = out[:, H:]).
        The connector is an fp32 GEMM; gradients flow into it and into the image features."""
        if image_features.dim() != 2:
            raise NotImplementedError("captioning from spatial image features (embedding_type spatial) is outside the implemented "
                                      "path: it needs flat image features [B, E]")
        out = ops.linear_f32(image_features.contiguous(), self.connector.weight, self.connector.bias)
        Hd = self.hidden_dim
        return out[:, :Hd].contiguous(), out[:, Hd:].contiguous()

    def init_hidden(self, batch_size, image_features=None):
        """reference :671-688 -> (h0, c0), each [1, B, H]: zeros, or the connector's state of ``image_features``."""
        if image_features is not None:
            h0, c0 = self.initial_state(image_features)
            return h0.unsqueeze(0), c0.unsqueeze(0)
        d = 2 if self.text_encoder == "bilstm" else 1
        z = torch.zeros(d * self.lstm.num_layers, batch_size, self.hidden_dim, device=self.lstm.weight_hh_l0.device)
        return z, z.clone()

    def forward(self, x, x_len, image_features=None, image_feature_map=None):
        attns = None
        if self.dropout_o and self.training:
            raise NotImplementedError("output dropout > 0 is not used by any contrastive configuration")
        if image_feature_map is not None:
            raise NotImplementedError("attention language models are outside the implemented path")
        if image_features is not None:                                      # captioning: image-initialised LSTM (:513-520)
            if not self.captioning:
                raise ValueError("image_features are only used by a captioning text encoder")
            h0, c0 = self.initial_state(image_features)
            if self.training or torch.is_grad_enabled():
                ret, raw_output = text_train.lstm_text_train(self.embedding.weight, self.lstm, x, x_len, self.dropout_i,
                                                             self.training, h0, c0)
            else:
                ret, raw_output = ops.lstm_text(self.embedding.weight, self.lstm, x, x_len, h0, c0)
            return ret, raw_output, attns
        spatial = self.embedding_type == "spatial"
        if self.text_encoder == "embedding" and spatial:
            # per-word embeddings are the features (reference :499, :579-580); differentiable gather
            B, L = x.shape
            raw_output = text_train.EmbedGatherPos.apply(self.embedding.weight, None, x).view(B, L, self.embedding_dim)
            ret = raw_output
        elif self.text_encoder == "embedding":
            ret, raw_output = ops.embed_meanpool(self.embedding.weight, x, x_len, True)       # reference :496-503
        elif self.text_encoder == "cbow":                                                    # reference :505-511
            assert spatial, "cbow with flat embedding is nonsense"
            raw_output = text_train.cbow_text_train(self.embedding.weight, x, self.crange)
            ret = raw_output
        elif self.text_encoder == "bilstm":                                                  # reference :513-552
            ret, raw_output = text_train.bilstm_text_train(self.embedding.weight, self.lstm, x, x_len, self.dropout_i,
                                                           self.training)
        elif self.text_encoder == "lstm":                                                    # reference :513-552
            if self.training or torch.is_grad_enabled():
                # differentiable path: embedding -> LockedDropout(dropout_i) -> LSTM (BPTT in the backward)
                ret, raw_output = text_train.lstm_text_train(self.embedding.weight, self.lstm, x, x_len, self.dropout_i,
                                                             self.training)
            else:
                ret, raw_output = ops.lstm_text(self.embedding.weight, self.lstm, x, x_len)
        elif self.text_encoder == "transformer":                                             # reference :553-573
            pos = self.pos_embed if self.pos_embed_type in ("sinusoidal", "learned") else None
            layer = self.transformer_encoder.layers[0]
            if self.training or torch.is_grad_enabled():
                ret, raw_output = text_train.transformer_text_train(self.embedding.weight, layer, pos, x, x_len, self.training,
                                                                    split=bool(getattr(self, "fp32_split", False)))
            else:
                ret, raw_output = ops.transformer_text(self.embedding.weight, layer, pos, x, x_len)
        else:
            raise NotImplementedError(f"text encoder {self.text_encoder!r} is outside the contrastive hot path")
        if spatial and self.text_encoder != "embedding":
            ret = raw_output                                                                  # reference :579-580
        return ret, raw_output, attns

    def _forward_unbatched(self, x, x_len, image_features=None):
        """reference :586-668: every utterance on its own (batch of one, trimmed to its length), stacked back; flat
        embeddings -> [B, E], spatial -> [B, L, E] zero-padded.  Used by the reference's batched == unbatched tests."""
        outs = []
        L = x.shape[1]
        for i in range(x.shape[0]):
            n = int(x_len[i])
            ret, _out, _a = self.forward(x[i:i + 1, :n].contiguous(), x_len[i:i + 1])
            ret = ret.squeeze(0)
            if self.embedding_type == "spatial" and ret.shape[0] < L:
                ret = torch.cat([ret, ret.new_zeros(L - ret.shape[0], ret.shape[1])], 0)
            outs.append(ret)
        return torch.stack(outs)

    @property
    def vocab_size(self):
        return len(self.vocab)

    @property
    def regressional(self):
        return self.text_encoder == "lstm"

    @property
    def captioning(self):
        return getattr(self, "_captioning", False)

    @property
    def has_attention(self):
        return getattr(self, "_attention", False)

    @property
    def has_attention_gate(self):
        return getattr(self, "_attention_gate", False)


class MultiModalModel(nn.Module):
    """encode_image / encode_text / forward / calculate_contrastive_loss (reference :691-822)."""

    def __init__(self, vision_encoder, text_encoder, args):
        super().__init__()
        self.args = vars(args) if args is not None else {}
        self.sim = self.args.get("sim", SIM)
        self.embedding_type = self.args.get("embedding_type", EMBEDDING_TYPE)
        self.normalize_features = self.args.get("normalize_features", NORMALIZE_FEATURES)
        self.initial_temperature = self.args.get("temperature", TEMPERATURE)
        self.fix_temperature = self.args.get("fix_temperature", FIX_TEMPERATURE)
        self.global_negatives = not self.args.get("local_negatives", False)
        self.image_embed = vision_encoder
        self.text_embed = text_encoder
        # reference :712-715 -- plain CPU tensor when fixed (not a buffer, not in the state_dict), Parameter otherwise
        self.logit_neg_log_temperature = torch.ones([]) * -np.log(self.initial_temperature)
        if not self.fix_temperature:
            self.logit_neg_log_temperature = nn.Parameter(self.logit_neg_log_temperature)
            self.logit_neg_log_temperature._cvcl_replicated_grad = True
        self._temp_dev = None

    @staticmethod
    def add_to_argparse(parser):
        parser.add_argument("--embedding_type", type=str, default=EMBEDDING_TYPE, choices=["spatial", "flat"])
        parser.add_argument("--embedding_dim", type=int, default=EMBEDDING_DIM)
        parser.add_argument("--normalize_features", action="store_true")
        parser.add_argument("--sim", type=str, default=SIM, choices=["mean", "max"])
        parser.add_argument("--temperature", type=float, default=TEMPERATURE)
        parser.add_argument("--fix_temperature", action="store_true")
        parser.add_argument("--local_negatives", action="store_true",
                            help="data-parallel runs: per-rank B x B loss with averaged gradients (Lightning DDP "
                                 "behaviour) instead of all-gathered global negatives")

    def _temperature_on(self, device):
        t = self.logit_neg_log_temperature
        if isinstance(t, nn.Parameter) or t.device == device:
            return t
        if self._temp_dev is None or self._temp_dev.device != device:
            self._temp_dev = t.to(device=device, dtype=torch.float32)       # one-time copy of the fixed scalar
        return self._temp_dev

    def encode_image(self, image):
        image_features, image_feature_map = self.image_embed(image)
        if self.normalize_features:
            if image_features.dim() == 4:            # spatial: F.normalize(dim=1) = per location over E (NHWC rows underneath)
                B, E, Hh, Ww = image_features.shape
                rows = ops.l2_normalize(image_features.permute(0, 2, 3, 1).reshape(B * Hh * Ww, E))
                image_features = rows.view(B, Hh, Ww, E).permute(0, 3, 1, 2)
            else:
                image_features = ops.l2_normalize(image_features)           # reference :736
        return image_features, image_feature_map

    def encode_text(self, text, text_length):
        text_features, text_outputs, attns = self.text_embed(text, text_length)
        if self.normalize_features:
            if text_features.dim() == 3:             # spatial: per word over E
                B, L, E = text_features.shape
                text_features = ops.l2_normalize(text_features.reshape(B * L, E)).view(B, L, E)
            else:
                text_features = ops.l2_normalize(text_features)              # reference :743
        return text_features, text_outputs

    def forward(self, image, text, text_length, return_image_features=False, return_text_outputs=False):
        image_features, image_feature_map = self.encode_image(image)
        text_features, text_outputs = self.encode_text(text, text_length)
        if self.embedding_type == "spatial":                                 # reference :757-780
            Bi, E, Hh, Ww = image_features.shape
            Bt, L, _ = text_features.shape
            rows_i = image_features.permute(0, 2, 3, 1).reshape(Bi * Hh * Ww, E)
            rows_t = text_features.reshape(Bt * L, E)
            if self.training and self.global_negatives and parallel.is_distributed():
                # global negatives: the per-location / per-word rows and the lengths of every rank, rank-major; every rank
                # evaluates the replicated N_g x N_g spatial logits and back-propagates into its own rows (SUM over ranks).
                # L is the pad length of THIS rank's batch (the collate pads to the batch's longest utterance), so the word rows
                # are first padded with zero rows to the rank-invariant length every rank knows without a collective
                # (parallel.common_text_length): a zero row adds 0 to both similarities, which sum over all L positions
                # (reference :763-777) -- the value is the reference's on the concatenated batch padded to any common L.
                Lg = parallel.common_text_length(L)
                if Lg != L:
                    rows_t = torch.nn.functional.pad(rows_t.view(Bt, L, E), (0, 0, 0, Lg - L)).reshape(Bt * Lg, E)
                    L = Lg
                world = parallel.world_size()
                parallel.check_spatial_global_bytes(Bi * world * Hh * Ww, Bt * world * L, self.sim, rows_i.device)
                rows_i = parallel.gather_rows(rows_i.view(Bi, Hh * Ww * E)).view(-1, E)
                rows_t = parallel.gather_rows(rows_t.view(Bt, L * E)).view(-1, E)
                text_length = parallel.gather_rows(text_length)
                Bi, Bt = Bi * world, Bt * world
            nlt = self._temperature_on(rows_i.device)
            if self.sim == "max":        # best location per word, summed over all L positions, / len
                logits_per_image = ops.spatial_max_logits(rows_i, rows_t, text_length, nlt, Bi, Hh * Ww, Bt, L)
            elif self.sim == "mean":     # sum of all location x word products / (H W len) = <mean location, sum words / len>
                hw = torch.full((Bi,), Hh * Ww, dtype=torch.int64, device=rows_i.device)
                pi = text_train.SeqSumDiv.apply(rows_i, hw, Bi, Hh * Ww)
                pt = text_train.SeqSumDiv.apply(rows_t, text_length, Bt, L)
                logits_per_image = ops.sim_logits(pi, pt, nlt)
            else:
                raise ValueError(self.sim)
            logits_per_text = logits_per_image.t()
            ret = logits_per_image, logits_per_text
            if return_image_features:
                ret = ret + (image_features, image_feature_map)
            if return_text_outputs:
                ret = ret + (text_outputs,)
            return ret
        fi, ft = image_features, text_features
        if self.training and self.global_negatives and parallel.is_distributed():
            # one RCCL all-gather over xGMI of the stacked features, the N_g x N_g logits, own-row gradient products backward
            logits_per_image = parallel.global_sim_logits(fi, ft, self._temperature_on(fi.device))
        else:
            logits_per_image = ops.sim_logits(fi, ft, self._temperature_on(fi.device))   # reference :755, :783-786
        logits_per_text = logits_per_image.t()                               # reference :787 (bitwise the same values)
        ret = logits_per_image, logits_per_text
        if return_image_features:
            ret = ret + (image_features, image_feature_map)
        if return_text_outputs:
            ret = ret + (text_outputs,)
        return ret

    def attention_maps(self, image, text, text_length, pairs="all", resize=False):
        """Grad-CAM maps of the images w.r.t. the texts' features, from the SAME encoder pass as the logits (flat ResNeXt
        encoder): -> (logits_per_image, logits_per_text, maps).  The targets are the text features as the logits use them
        (L2-normalised with normalize_features), and the maps those of gradCAM(image_embed.model, image, target, layer4,
        normalize_features) -- see attention_maps.gradCAM_pairs for ``pairs`` and ``resize``.  Evaluation use: run it under
        torch.no_grad(); the logits are those of forward() on the same inputs."""
        from .attention_maps import _resnet_of, gradcam_from_features
        resnet = _resnet_of(self.image_embed)
        features, feature_map = self.image_embed(image)
        fi = ops.l2_normalize(features) if self.normalize_features else features          # as encode_image
        ft, _ = self.encode_text(text, text_length)
        logits_per_image = ops.sim_logits(fi, ft, self._temperature_on(fi.device))
        size = tuple(image.shape[2:]) if resize is True else resize
        maps = gradcam_from_features(feature_map, features, resnet.fc.weight, ft, self.normalize_features, pairs, size)
        return logits_per_image, logits_per_image.t(), maps

    def self_attention_maps(self, image, text, text_length):
        """ViT encoder: -> (logits_per_image, logits_per_text, maps [N, gh, gw]) -- the logits of forward() on the same inputs and
        the CLS token's last-block self-attention over the patch grid, averaged over the heads (attention_maps.vit_cls_attention).
        The maps depend on the image alone, not on the text (unlike Grad-CAM, which stays undefined for the ViT).  Evaluation use."""
        from .attention_maps import vit_cls_attention
        maps = vit_cls_attention(self.image_embed, image)      # (refuses a ResNeXt encoder before any encoder pass)
        logits_per_image, logits_per_text = self(image, text, text_length)
        return logits_per_image, logits_per_text, maps

    def attention_rollout_maps(self, image, text, text_length, head_fusion="mean", start_layer=0):
        """self_attention_maps with the CLS token's attention rollout over all blocks in place of the last block's CLS row
        (attention_maps.vit_attention_rollout): -> (logits_per_image, logits_per_text, maps [N, gh, gw])."""
        from .attention_maps import vit_attention_rollout
        maps = vit_attention_rollout(self.image_embed, image, head_fusion=head_fusion, start_layer=start_layer)
        logits_per_image, logits_per_text = self(image, text, text_length)
        return logits_per_image, logits_per_text, maps

    def calculate_contrastive_loss(self, x, y, y_len):
        logits_per_image, logits_per_text, image_features, image_feature_map, text_outputs = self(
            x, y, y_len, return_image_features=True, return_text_outputs=True)
        infonce_loss, m = ops.infonce(logits_per_image)                      # reference :801-818 in one kernel pass
        return infonce_loss, m[0], m[1], m[2], m[3], logits_per_image, logits_per_text, \
            image_features, image_feature_map, text_outputs


class LanguageModel(nn.Module):
    """Tied output layer + token-wise cross entropy (reference multimodal.py:825-890): the ``lambda_lm > 0`` branch of the
    joint loss.  The projection is an fp32 GEMM (LinearF32: its weight gradient adds into the tied embedding table), the
    loss ``cvcl_token_ce_fwd/bwd``.  Captioning LMs start the LSTM from the connector's state of the image features; beam-search
    decoding runs on HIP (plain and captioning LSTM LMs).  Attention decoders stay out of scope."""

    def __init__(self, text_encoder, args):
        super().__init__()
        self.args = vars(args) if args is not None else {}
        self.text_encoder = text_encoder
        self.output_layer = nn.Linear(text_encoder.hidden_dim, text_encoder.vocab_size, bias=self.args.get("bias", True))
        if self.args.get("tie", True):
            self.output_layer.weight = self.text_encoder.embedding.weight

    @staticmethod
    def add_to_argparse(parser):
        parser.add_argument("--tie", type=lambda s: bool(eval(s)), default=True)
        parser.add_argument("--bias", type=lambda s: bool(eval(s)), default=True)

    def forward(self, y, y_len, outputs=None, image_features=None, image_feature_map=None):
        if image_feature_map is not None:
            raise NotImplementedError("attention language models are outside the implemented path")
        te = self.text_encoder
        if image_features is not None and outputs is None:
            _feat, outputs, _attns = te(y, y_len, image_features=image_features)
        elif te.text_encoder == "embedding":
            # per-word embeddings, gathered differentiably (the mean-pool op marks its per-word output non-differentiable)
            B, L = y.shape
            outputs = text_train.EmbedGatherPos.apply(te.embedding.weight, None, y).view(B, L, te.embedding_dim)
        elif outputs is None:
            _feat, outputs, _attns = te(y, y_len)
        B, L, E = outputs.shape
        logits = ops.linear_f32(outputs.reshape(B * L, E), self.output_layer.weight, self.output_layer.bias)   # :859
        return outputs, logits.view(B, L, -1), None

    def calculate_ce_loss(self, y, y_len, outputs=None, image_features=None, image_feature_map=None, tokenwise=False,
                          weight=None):
        if weight is not None:
            raise NotImplementedError("class weights are not used by any reference configuration")
        te = self.text_encoder
        if te.regressional:                                  # predict token l+1 from position l (:879-883)
            if te.text_encoder != "embedding" and outputs is None:
                _feat, outputs, _attns = te(y, y_len, image_features=image_features)
            outputs_in = outputs[:, :-1].contiguous() if outputs is not None else None
            outs, logits, attns = self(y[:, :-1], y_len, outputs=outputs_in)
            labels = y[:, 1:1 + logits.size(1)].contiguous()
            outputs = outputs if outputs is not None else outs
        else:
            outputs, logits, attns = self(y, y_len, outputs=outputs)
            labels = y.contiguous()
        B, Lp, V = logits.shape
        loss = ops.token_cross_entropy(logits.reshape(B * Lp, V), labels.reshape(-1), PAD_TOKEN_ID)
        if tokenwise:
            loss = loss.view(B, Lp)
        else:                                                # reduction "mean" over the non-ignored tokens
            loss = ops.lm_loss_summaries(loss, labels.reshape(-1))[0][0]
        return loss, outputs, logits, attns, labels

    def beam_search_decode(self, batch_size, beam_width, decode_length, length_penalty_alpha, image_features=None,
                           image_feature_map=None):
        """reference :893-960 -> (beam_seq [B, K, steps + 1] int64, log_prob [B, K]).  Plain LSTM LMs start from zeros,
        captioning ones from the connector's state of ``image_features`` [B, E].  One HIP launch chain per step with the stop
        test on the device (ops.beam_search_lstm)."""
        te = self.text_encoder
        assert te.regressional, "only regressional text encoder supports beam search decoding"
        if image_feature_map is not None or te.has_attention:
            raise NotImplementedError("attention language models are outside the implemented path")
        h0 = c0 = None
        if image_features is not None:
            if not te.captioning:
                raise ValueError("image_features are only used by a captioning text encoder")
            with torch.no_grad():
                h0, c0 = te.initial_state(image_features.detach())
        bias = self.output_layer.bias
        return ops.beam_search_lstm(te.embedding.weight, te.lstm, self.output_layer.weight, bias, batch_size, beam_width,
                                    decode_length, length_penalty_alpha, h0, c0, sos_id=SOS_TOKEN_ID, eos_id=EOS_TOKEN_ID)


def calculate_attn_reg_loss(attns):
    raise NotImplementedError("attention regularisation is outside the contrastive hot path")
