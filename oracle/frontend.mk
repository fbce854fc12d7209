# oracle/frontend.mk -- builds oracle/_ref/libsummertts_frontend.so: the REFERENCE's own host text frontend (north_star: "the
# text frontend (TN/hz2py/g2p) stays on host C++"), compiled IN PLACE from $(REF) with the reference's flags
# (CMakeLists.txt:8-9) and wrapped by frontend/frontend_shim.cpp (this repo's code: the blob-section walk of
# SynthesizerTrn.cpp:165-297 and the text -> phoneme-id call sequence of SynthesizerTrn.cpp:327-355).
#
# No reference source is copied; the output lies under oracle/_ref/ (git-ignored), next to oracle/Makefile's compiled reference,
# and travels to the GPU box with it.  The library is OPTIONAL: libsummertts_hip.so dlopen()s it when a model blob carries
# frontend sections; without it SynthesizerTrn::infer keeps accepting phoneme ids as text.  Needs the
# reference (absent on the GPU box).
#
#   make -C oracle -f frontend.mk        -> _ref/libsummertts_frontend.so and _ref/fe_obj/test/main.o (the reference's unmodified demo
#                                           caller, compiled against its own headers; tests/test_frontend_cpu.py links it)
REF      ?= /root/reference
OUT      := _ref
OBJDIR   := $(OUT)/fe_obj
SHIM     := ../frontend/frontend_shim.cpp
CXX      ?= g++
FLAGS    := -O3 -fopenmp -std=c++11 -fPIC -w
TABFLAGS := -O0 -std=c++11 -fPIC -w     # the two 125 000-line pronunciation tables: nothing to optimise
INC      := -I$(REF)/eigen-3.4.0 -I$(REF)/src/tn/header -I$(REF)/include -I$(REF)/src/header

TN_SRCS  := $(addprefix $(REF)/src/tn/glog/src/,demangle.cc logging.cc raw_logging.cc symbolize.cc utilities.cc vlog_is_on.cc signalhandler.cc) \
            $(addprefix $(REF)/src/tn/gflags/src/,gflags.cc gflags_reporting.cc gflags_completions.cc) \
            $(addprefix $(REF)/src/tn/openfst/src/lib/,compat.cc flags.cc fst.cc fst-types.cc mapped-file.cc properties.cc symbol-table.cc symbol-table-ops.cc util.cc weight.cc) \
            $(addprefix $(REF)/src/tn/,processor.cc token_parser.cc utf8_string.cc)
FE_SRCS  := $(addprefix $(REF)/src/engipa/,EnglishText2Id.cpp InitIPASymbols.cpp) \
            $(addprefix $(REF)/src/hz2py/,hanzi2phoneid.cpp Hanz2Piny.cpp pinyinmap.cpp) \
            $(addprefix $(REF)/src/nn_op/,nn_sigmoid.cpp nn_tanh.cpp)
TAB_SRCS := $(addprefix $(REF)/src/engipa/,alphabet.cpp ipa.cpp)

obj = $(patsubst $(REF)/src/%,$(OBJDIR)/%.o,$(1))
OBJS := $(call obj,$(TN_SRCS)) $(call obj,$(FE_SRCS))
TABS := $(call obj,$(TAB_SRCS))

.PHONY: all clean
all: $(OUT)/libsummertts_frontend.so $(OBJDIR)/test/main.o
$(TABS): $(OBJDIR)/%.o: $(REF)/src/%
	@mkdir -p $(dir $@)
	$(CXX) $(TABFLAGS) $(INC) -c $< -o $@
$(OBJS): $(OBJDIR)/%.o: $(REF)/src/%
	@mkdir -p $(dir $@)
	$(CXX) $(FLAGS) $(INC) -c $< -o $@
$(OBJDIR)/frontend_shim.o: $(SHIM)
	@mkdir -p $(dir $@)
	$(CXX) $(FLAGS) $(INC) -c $< -o $@
$(OBJDIR)/test/main.o: $(REF)/test/main.cpp
	@mkdir -p $(dir $@)
	$(CXX) -O1 -std=c++11 -w -I$(REF)/include -I$(REF)/src/header -c $< -o $@
$(OUT)/libsummertts_frontend.so: $(OBJS) $(TABS) $(OBJDIR)/frontend_shim.o
	$(CXX) -shared -fopenmp -o $@ $^ -lpthread
clean:
	rm -rf $(OBJDIR) $(OUT)/libsummertts_frontend.so
